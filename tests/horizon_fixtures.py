"""The long-horizon golden vectors (tests/golden/make_golden_horizon.py) as a whole model's state, inputs and gradients.

The fixtures store the two time-embedding tables and their gradients as the rows H and D select; `load` rebuilds the
full [24 | 7, R*N*T_out] tables with zeros elsewhere (rows that cannot influence the forward and receive no gradient)."""
import numpy as np
import torch

from conftest import load_golden

# name, factory, components R, input channels C, T_in, T_out, nodes N, dilations of the two blocks (msgat.py:220-226)
CASES = [
    ("msgat72_to24_n32.npz", "msgat72", 3, 3, 12, 24, 32),
    ("msgat48_to40_n23.npz", "msgat48", 2, 1, 8, 40, 23),
    ("msgat48_to64_n24.npz", "msgat48", 1, 2, 16, 64, 24),
]
DILATIONS = ([1, 2], [2, 4])
TABLES = {"te.h_ebd.weight": ("H", 24), "te.d_ebd.weight": ("D", 7)}


def load(name):
    """-> (golden arrays, state_dict {name: tensor}, gradients {parameter name: np.ndarray}); X and Y as float32."""
    g = load_golden(name)
    g["X"], g["Y"] = g["X"].astype(np.float32), g["Y"].astype(np.float32)
    state = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")}
    grads = {k[2:]: v for k, v in g.items() if k.startswith("g.")}
    for key, (idx, rows) in TABLES.items():
        sel = torch.from_numpy(g[idx])
        width = g[f"rows.{key}"].shape[1]
        full, dfull = torch.zeros(rows, width), np.zeros((rows, width), np.float32)
        full[sel] = torch.from_numpy(g[f"rows.{key}"])
        dfull[g[idx]] = g[f"grows.{key}"]
        state[key], grads[key] = full, dfull
    return g, state, grads
