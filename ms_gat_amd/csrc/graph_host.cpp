// Host side of the boundary: dense [N,N] adjacency -> CSR + CSC.
//
// The reference keeps the adjacency dense (built at data_loader.py:59-66, held as a
// frozen parameter at msgat.py:190) and applies it as a mask `att * adjacency`
// (attention.py:36).  Only its non-zeros matter to that product, so the kernels walk
// them: CSR for the forward gather, CSC (+ the CSC->CSR permutation) for the transposed
// gather of the backward pass.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "msgat_hip.h"

static inline bool is_edge(float v) { return !(v == 0.0f); }  // NaN is an edge (it would poison the dense product too)

extern "C" int msgat_graph_count(const float* adj, int32_t n, int64_t ld, int32_t* nnz_out) {
  if (!adj || !nnz_out) return MSGAT_ERR_NULL;
  if (n <= 0 || ld < n) return MSGAT_ERR_SHAPE;
  int64_t cnt = 0;
  for (int32_t i = 0; i < n; ++i) {
    const float* row = adj + (int64_t)i * ld;
    for (int32_t j = 0; j < n; ++j) cnt += is_edge(row[j]) ? 1 : 0;
  }
  if (cnt > INT32_MAX) return MSGAT_ERR_SHAPE;
  *nnz_out = (int32_t)cnt;
  return MSGAT_OK;
}

extern "C" int msgat_graph_build(const float* adj, int32_t n, int64_t ld, int32_t nnz,
                                 int32_t* rowptr, int32_t* col, float* val, int32_t* erow,
                                 int32_t* colptr, int32_t* crow, int32_t* cperm, int32_t* cpos) {
  if (!adj || !rowptr || !colptr) return MSGAT_ERR_NULL;
  if (nnz > 0 && (!col || !val || !erow || !crow || !cperm || !cpos)) return MSGAT_ERR_NULL;
  if (n <= 0 || ld < n || nnz < 0) return MSGAT_ERR_SHAPE;

  // CSR, rows in order, columns ascending inside a row
  std::vector<int32_t> colcount((size_t)n + 1, 0);
  int64_t e = 0;
  for (int32_t i = 0; i < n; ++i) {
    rowptr[i] = (int32_t)e;
    const float* row = adj + (int64_t)i * ld;
    for (int32_t j = 0; j < n; ++j) {
      if (!is_edge(row[j])) continue;
      if (e >= nnz) return MSGAT_ERR_SHAPE;  // caller's count is stale
      col[e] = j;
      val[e] = row[j];
      erow[e] = i;
      colcount[(size_t)j + 1]++;
      ++e;
    }
  }
  if (e != nnz) return MSGAT_ERR_SHAPE;
  rowptr[n] = nnz;

  // CSC by counting sort over the CSR edges: rows ascending inside a column
  colptr[0] = 0;
  for (int32_t j = 0; j < n; ++j) colptr[j + 1] = colptr[j] + colcount[(size_t)j + 1];
  std::vector<int32_t> cursor(colptr, colptr + n);
  for (int32_t k = 0; k < nnz; ++k) {
    const int32_t pos = cursor[col[k]]++;
    crow[pos] = erow[k];
    cperm[pos] = k;
    cpos[k] = pos;
  }
  return MSGAT_OK;
}

// CSC (+ both permutations) of a finished CSR: counting sort over the edges, rows ascending inside a column
static void build_csc(int32_t n, int32_t nnz, const int32_t* col, const int32_t* erow, int32_t* colptr, int32_t* crow,
                      int32_t* cperm, int32_t* cpos) {
  colptr[0] = 0;
  for (int32_t j = 0; j <= n; ++j) colptr[j] = 0;
  for (int32_t k = 0; k < nnz; ++k) colptr[col[k] + 1]++;
  for (int32_t j = 0; j < n; ++j) colptr[j + 1] += colptr[j];
  std::vector<int32_t> cursor(colptr, colptr + n);
  for (int32_t k = 0; k < nnz; ++k) {
    const int32_t pos = cursor[col[k]]++;
    crow[pos] = erow[k];
    cperm[pos] = k;
    cpos[k] = pos;
  }
}

// A sparse adjacency brings its pattern as indices: every stored index is an edge, an explicit 0 included (its value
// is a weight that may become non-zero later), and [n,n] is never formed (n = 200 000 is 160 GB of floats).
extern "C" int msgat_graph_build_indices(const int32_t* in_rowptr, const int32_t* in_col, int32_t n, int32_t nnz,
                                         int32_t* rowptr, int32_t* col, int32_t* erow, int32_t* colptr, int32_t* crow,
                                         int32_t* cperm, int32_t* cpos, int32_t* order) {
  if (!in_rowptr || !rowptr || !colptr) return MSGAT_ERR_NULL;
  if (nnz > 0 && (!in_col || !col || !erow || !crow || !cperm || !cpos || !order)) return MSGAT_ERR_NULL;
  if (n <= 0 || nnz < 0) return MSGAT_ERR_SHAPE;
  if (in_rowptr[0] != 0 || in_rowptr[n] != nnz) return MSGAT_ERR_GRAPH;
  for (int32_t i = 0; i < n; ++i)
    if (in_rowptr[i + 1] < in_rowptr[i]) return MSGAT_ERR_GRAPH;
  std::vector<std::pair<int32_t, int32_t>> row;   // (column, input index) of one row
  for (int32_t i = 0; i < n; ++i) {
    const int32_t b = in_rowptr[i], e = in_rowptr[i + 1];
    rowptr[i] = b;
    row.clear();
    for (int32_t k = b; k < e; ++k) {
      if (in_col[k] < 0 || in_col[k] >= n) return MSGAT_ERR_GRAPH;
      row.emplace_back(in_col[k], k);
    }
    std::sort(row.begin(), row.end());
    for (size_t k = 0; k < row.size(); ++k) {
      if (k > 0 && row[k].first == row[k - 1].first) return MSGAT_ERR_GRAPH;   // a column stored twice
      col[b + k] = row[k].first;
      order[b + k] = row[k].second;
      erow[b + k] = i;
    }
  }
  rowptr[n] = nnz;
  build_csc(n, nnz, col, erow, colptr, crow, cperm, cpos);
  return MSGAT_OK;
}

extern "C" int msgat_graph_validate(const msgat_graph_t* g) {
  if (!g || !g->rowptr || !g->colptr) return MSGAT_ERR_NULL;
  const int32_t n = g->n_nodes, nnz = g->nnz;
  if (n <= 0 || nnz < 0) return MSGAT_ERR_SHAPE;
  if (nnz > 0 && (!g->col || !g->val || !g->erow || !g->crow || !g->cperm || !g->cpos)) return MSGAT_ERR_NULL;
  if (g->rowptr[0] != 0 || g->rowptr[n] != nnz || g->colptr[0] != 0 || g->colptr[n] != nnz)
    return MSGAT_ERR_GRAPH;
  for (int32_t i = 0; i < n; ++i) {
    if (g->rowptr[i + 1] < g->rowptr[i] || g->colptr[i + 1] < g->colptr[i]) return MSGAT_ERR_GRAPH;
    for (int32_t k = g->rowptr[i]; k < g->rowptr[i + 1]; ++k) {
      if (g->col[k] < 0 || g->col[k] >= n || g->erow[k] != i) return MSGAT_ERR_GRAPH;
      if (k > g->rowptr[i] && g->col[k] <= g->col[k - 1]) return MSGAT_ERR_GRAPH;
    }
  }
  std::vector<char> seen((size_t)nnz, 0);
  for (int32_t j = 0; j < n; ++j) {
    for (int32_t k = g->colptr[j]; k < g->colptr[j + 1]; ++k) {
      const int32_t p = g->cperm[k];
      if (p < 0 || p >= nnz || seen[(size_t)p]) return MSGAT_ERR_GRAPH;
      seen[(size_t)p] = 1;
      if (g->col[p] != j || g->erow[p] != g->crow[k] || g->cpos[p] != k) return MSGAT_ERR_GRAPH;
    }
  }
  // SELL forms: every CSR edge sits at exactly one position, in the lane that owns the row the edge starts from
  // (rows form) or the column it ends in (columns form), as that lane's k-th entry in CSR / CSC order, and holds
  // the node at the edge's other end; everything else is padding
  for (int form = 0; form < 2; ++form) {
    const msgat_sell_t& j = form == 0 ? g->sell_rows : g->sell_cols;
    if (j.n_slices == 0) continue;
    if (j.n_slices != (n + 63) / 64 || j.n_pos < nnz || !j.slice_off || !j.lane_row) return MSGAT_ERR_GRAPH;
    if (!j.idx || !j.src) return MSGAT_ERR_NULL;  // read below whatever n_pos is (padding entries, the slack)
    if (j.slice_off[0] != 0 || j.slice_off[j.n_slices] != j.n_pos) return MSGAT_ERR_GRAPH;
    const int32_t* ptr = form == 0 ? g->rowptr : g->colptr;
    std::vector<char> used((size_t)nnz, 0), seen_row((size_t)n, 0);
    int32_t prev_deg = INT32_MAX;
    for (int32_t s = 0; s < j.n_slices; ++s) {
      const int32_t span = j.slice_off[s + 1] - j.slice_off[s];
      if (span < 0 || span % 256 != 0) return MSGAT_ERR_GRAPH;  // 64 lanes x a multiple of 4 columns
      const int32_t width = span / 64;
      for (int32_t l = 0; l < 64; ++l) {
        const int32_t owner = j.lane_row[64 * s + l];
        if (owner < -1 || owner >= n) return MSGAT_ERR_GRAPH;
        int32_t deg = 0;
        if (owner >= 0) {
          if (seen_row[(size_t)owner]) return MSGAT_ERR_GRAPH;
          seen_row[(size_t)owner] = 1;
          deg = ptr[owner + 1] - ptr[owner];
          if (deg > prev_deg || deg > width) return MSGAT_ERR_GRAPH;  // sorted by degree, descending
          prev_deg = deg;
        }
        for (int32_t k = 0; k < width; ++k) {
          const int32_t p = j.slice_off[s] + 256 * (k >> 2) + 4 * l + (k & 3), e = j.src[p];
          if (k >= deg) {
            if (e != -1 || j.idx[p] >= n) return MSGAT_ERR_GRAPH;
            continue;
          }
          if (e < 0 || e >= nnz || used[(size_t)e]) return MSGAT_ERR_GRAPH;
          used[(size_t)e] = 1;
          // some edge of the owner's row (rows form) / column (columns form): which one sits in which column is the
          // builder's choice (it picks the order with the fewest LDS bank conflicts)
          const int32_t from = form == 0 ? g->erow[e] : g->col[e];
          const int32_t to = form == 0 ? g->col[e] : g->erow[e];
          if (from != owner || j.idx[p] != to) return MSGAT_ERR_GRAPH;
          if (j.pos && j.pos[e] != p) return MSGAT_ERR_GRAPH;
        }
      }
    }
    int32_t pair = 0;
    for (int32_t i = 0; 2 * i < j.n_slices; ++i) {
      const int32_t o = j.n_slices - 1 - i;
      pair = std::max(pair, (j.slice_off[i + 1] - j.slice_off[i]) / 256 + (o > i ? (j.slice_off[o + 1] - j.slice_off[o]) / 256 : 0));
    }
    if (j.pair_trips != pair) return MSGAT_ERR_GRAPH;
    for (int32_t i = 0; i < n; ++i)
      if (!seen_row[(size_t)i]) return MSGAT_ERR_GRAPH;
    for (int32_t e = 0; e < nnz; ++e)
      if (!used[(size_t)e]) return MSGAT_ERR_GRAPH;
    for (int32_t p = j.n_pos; p < j.n_pos + MSGAT_SELL_SLACK; ++p)
      if (j.idx[p] >= n) return MSGAT_ERR_GRAPH;  // the slack is read (and ignored) by the kernels
  }
  return MSGAT_OK;
}

// ---- sliced ELLPACK (SELL-64, degree-sorted) layout of one sparse structure: see msgat_sell_t ---------------------
// order = rows by degree, descending, stable (counting sort); slice s = order[64 s .. 64 s + 63]; its width is the
// degree of its first row rounded up to a multiple of 4; a "trip" = 4 consecutive columns, stored lane-interleaved
// (lane l owns entries 4 l .. 4 l + 3 of the trip's 256) so one 16-B-per-lane load fetches a lane's 4 edges.
static void sell_order(const int32_t* ptr, int32_t n, std::vector<int32_t>& order) {
  int32_t maxdeg = 0;
  for (int32_t i = 0; i < n; ++i) maxdeg = std::max(maxdeg, ptr[i + 1] - ptr[i]);
  std::vector<int32_t> start((size_t)maxdeg + 2, 0);
  for (int32_t i = 0; i < n; ++i) start[(size_t)(maxdeg - (ptr[i + 1] - ptr[i])) + 1]++;
  for (int32_t d = 0; d <= maxdeg; ++d) start[(size_t)d + 1] += start[(size_t)d];
  order.assign((size_t)n, 0);
  for (int32_t i = 0; i < n; ++i) order[(size_t)start[(size_t)(maxdeg - (ptr[i + 1] - ptr[i]))]++] = i;
}

// the lane groups a ds_read_b128 is served in, one LDS cycle each when conflict-free (MI355X_MICROARCH.md, LDS)
static const int kSellGroups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

extern "C" int msgat_graph_sell_count(const int32_t* ptr, int32_t n, int32_t* n_slices_out, int32_t* n_pos_out,
                                      int32_t* pair_trips_out) {
  if (!ptr || !n_slices_out || !n_pos_out || !pair_trips_out) return MSGAT_ERR_NULL;
  if (n <= 0) return MSGAT_ERR_SHAPE;
  for (int32_t i = 0; i < n; ++i)
    if (ptr[i + 1] < ptr[i]) return MSGAT_ERR_GRAPH;
  std::vector<int32_t> order;
  sell_order(ptr, n, order);
  const int32_t ns = (n + 63) / 64;
  int64_t total = 0;
  std::vector<int32_t> trips((size_t)ns, 0);
  for (int32_t s = 0; s < ns; ++s) {
    const int32_t first = order[(size_t)64 * s];
    trips[(size_t)s] = (ptr[first + 1] - ptr[first] + 3) / 4;
    total += (int64_t)256 * trips[(size_t)s];
  }
  if (total > INT32_MAX - MSGAT_SELL_SLACK) return MSGAT_ERR_SHAPE;
  int32_t pair = 0;
  for (int32_t i = 0; 2 * i < ns; ++i)
    pair = std::max(pair, trips[(size_t)i] + (ns - 1 - i > i ? trips[(size_t)(ns - 1 - i)] : 0));
  *n_slices_out = ns;
  *n_pos_out = (int32_t)total;
  *pair_trips_out = pair;
  return MSGAT_OK;
}

extern "C" int msgat_graph_sell_build(const int32_t* ptr, const int32_t* idx, const int32_t* perm, int32_t n,
                                      int32_t nnz, int32_t n_slices, int32_t n_pos, int32_t* slice_off,
                                      int32_t* lane_row, uint16_t* sidx, int32_t* ssrc, int32_t* spos) {
  if (!ptr || !slice_off || !lane_row || !sidx) return MSGAT_ERR_NULL;
  if (n_pos > 0 && !ssrc) return MSGAT_ERR_NULL;
  if (nnz > 0 && !idx) return MSGAT_ERR_NULL;
  if (n <= 0 || n > 65535 || nnz < 0 || n_slices != (n + 63) / 64 || ptr[n] != nnz || n_pos < nnz) return MSGAT_ERR_SHAPE;
  std::vector<int32_t> order;
  sell_order(ptr, n, order);
  int64_t off = 0;
  for (int32_t s = 0; s < n_slices; ++s) {
    const int32_t first = order[(size_t)64 * s];
    const int32_t width = (ptr[first + 1] - ptr[first] + 3) / 4 * 4;
    if (off + (int64_t)64 * width > n_pos) return MSGAT_ERR_SHAPE;  // caller's count is stale
    slice_off[s] = (int32_t)off;
    // which of a row's edges goes to which column is free (a row's sum does not care), and it decides the LDS bank
    // conflicts of the kernels' gathers: a ds_read_b128 serves its 64 lanes in 4 fixed groups of 16, one cycle per
    // group if the 16 addresses fall into 16 different bank quads (node index mod 16), one more per extra address
    // on a quad.  In CSR order the quads are random: 11.5 cycles per instruction at the stress graph (measured:
    // SQ_LDS_IDX_ACTIVE / SQ_INSTS_LDS; same figure from this model).  So every column is filled group by group
    // with a maximum bipartite matching lane -> quad over the lanes' remaining edges (Kuhn's algorithm, lanes with
    // the fewest edges left first); lanes the matching leaves out take their least loaded quad: 6.5 cycles.
    std::vector<int32_t> rem[64];   // remaining edges of each lane, CSR order
    int32_t rowof[64], degof[64];
    for (int32_t l = 0; l < 64; ++l) {
      const int32_t i = 64 * s + l;
      const int32_t row = i < n ? order[(size_t)i] : -1;
      lane_row[i] = row;
      rowof[l] = row;
      degof[l] = row >= 0 ? ptr[row + 1] - ptr[row] : 0;
      rem[l].clear();
      for (int32_t k = 0; k < degof[l]; ++k) rem[l].push_back(ptr[row] + k);
    }
    for (int32_t k = 0; k < width; ++k) {
      for (int32_t l = 0; l < 64; ++l) {  // padding by default: coefficient 0 times node 0
        const int32_t p = (int32_t)off + 256 * (k >> 2) + 4 * l + (k & 3);
        sidx[p] = 0;
        ssrc[p] = -1;
      }
      for (int grp = 0; grp < 4; ++grp) {
        int32_t active[16], na = 0;
        for (int i = 15; i >= 0; --i)  // descending lane index = fewest remaining edges first (rows are degree-sorted)
          if (!rem[kSellGroups[grp][i]].empty()) active[na++] = kSellGroups[grp][i];
        int32_t owner[16];
        for (int q = 0; q < 16; ++q) owner[q] = -1;
        bool seen[16];
        struct Kuhn {
          std::vector<int32_t>* rem;
          const int32_t* idx;
          int32_t* owner;
          bool* seen;
          bool run(int32_t l) {
            for (int q = 0; q < 16; ++q) {
              if (seen[q]) continue;
              bool has = false;
              for (int32_t e : rem[l]) has = has || ((idx[e] & 15) == q);
              if (!has) continue;
              seen[q] = true;
              if (owner[q] < 0 || run(owner[q])) { owner[q] = l; return true; }
            }
            return false;
          }
        } kuhn{rem, idx, owner, seen};
        for (int32_t a = 0; a < na; ++a) {
          for (int q = 0; q < 16; ++q) seen[q] = false;
          kuhn.run(active[a]);
        }
        int32_t cnt[16], quad_of_lane[64];
        for (int32_t a = 0; a < na; ++a) quad_of_lane[active[a]] = -1;
        for (int q = 0; q < 16; ++q) {
          cnt[q] = owner[q] >= 0 ? 1 : 0;
          if (owner[q] >= 0) quad_of_lane[owner[q]] = q;
        }
        for (int32_t a = 0; a < na; ++a) {
          const int32_t l = active[a];
          std::vector<int32_t>& r = rem[l];
          size_t pick = 0;
          if (quad_of_lane[l] >= 0) {
            while ((idx[r[pick]] & 15) != quad_of_lane[l]) ++pick;   // first remaining edge on the matched quad
          } else {
            for (size_t i = 1; i < r.size(); ++i)
              if (cnt[idx[r[i]] & 15] < cnt[idx[r[pick]] & 15]) pick = i;
            cnt[idx[r[pick]] & 15]++;
          }
          const int32_t e = r[pick];
          r.erase(r.begin() + (long)pick);
          const int32_t p = (int32_t)off + 256 * (k >> 2) + 4 * l + (k & 3);
          const int32_t id = perm ? perm[e] : e;
          sidx[p] = (uint16_t)idx[e];
          ssrc[p] = id;
          if (spos) spos[id] = p;
        }
      }
    }
    off += (int64_t)64 * width;
  }
  if (off != n_pos) return MSGAT_ERR_SHAPE;
  slice_off[n_slices] = n_pos;
  for (int32_t p = n_pos; p < n_pos + MSGAT_SELL_SLACK; ++p) sidx[p] = 0;
  return MSGAT_OK;
}
