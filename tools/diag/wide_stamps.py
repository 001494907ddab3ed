"""Development: per-phase cycles of the long-horizon kernel (tools/diag/libmpcqp_wstamps.so,
-DMPCQP_WIDE_STAMPS): python tools/diag/wide_stamps.py [N] [B]"""
import json, os, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[2]
os.environ.setdefault("MPCQP_LIB", str(ROOT / "tools" / "diag" / "libmpcqp_wstamps.so"))
os.environ.setdefault("MPCQP_ABI_ANY", "1")
sys.path[:0] = [str(ROOT / "rrt-mpc_amd"), str(ROOT / "oracle"), str(ROOT / "tests")]
import numpy as np
import torch
from gpu_helpers import d2h
from mpcqp import _lib, scenarios
from mpcqp.config import MPCConfig
from mpcqp.control.mpc_controller import BatchedMPCController
N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
b = scenarios.config3(B, horizon=N)
ctrl = BatchedMPCController(MPCConfig(horizon=N).to_parameters(0.8), B, device="cuda:0")
ctrl.solve_batch(b.x0, b.ref, b.u_prev)
torch.cuda.synchronize()
L = _lib.lib()
SS = L.mpcqp_state_stride(N)
st = d2h(L.mpcqp_state_buffer(ctrl._ws), np.zeros((B, SS)))
n = 2 * N
off = n * (n + 1)
names = ["setup", "admm.factor", "admm.iteration", "admm.check", "polish.form", "polish.sweep", "polish.solve",
         "polish.linesearch"]
S = st[:, off:off + 8].mean(axis=0)
it = ctrl._iters[:B].cpu().numpy().mean(axis=0)
print(json.dumps({"N": N, "B": B, "cycles_per_qp": dict(zip(names, S.round().tolist())), "iters_mean": it.tolist(),
                  "total": float(S.sum())}))
