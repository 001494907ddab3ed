#!/usr/bin/env python3
"""Per-QP parameter classes against what they replace ("Per-QP parameter classes").

Config-3 inputs, B = 4096, N = 20 (the headline workload), 100 warm and 100 timed steps per repeat,
timed with device events around the timed steps; the legs alternate within one process and each is
repeated five times.  Every leg goes through the C-ABI directly (create / build / solve on a ctypes
handle), so two libraries can be timed in one process with the same host code:

  plain          mpcqp_build + mpcqp_solve of this tree's library (the headline path)
  plain_parent   the same calls on another build of the library (--parent-lib: the parent commit's)
  mixed_k1       mpcqp_build_mixed with one class (the workspace's block) and cls = 0
  mixed_k9       mpcqp_build_mixed with the nine blocks of tests/param_variants.py, cls[b] = b % 9
  nine_plain     what a user did before: nine plain workspaces, one per block, solved one after another
                 on the same stream, each with the QPs of its class (the same QPs as mixed_k9)

With --class-pairing (N <= 15: mpcqp_set_class_pairing; --classes K takes the first K blocks) three more legs
join the rotation, and the slot kernel is timed on its own (mpcqp_class_slots over this batch, device events):

  mixed_kK_paired   the mixed launch with two QPs of one class per wave (the same bits as mixed_kK)
  K_plain_paired    the K plain workspaces under MPCQP_PAIR_ON: the paired launches a mixed one replaces

    python tools/mixed_bench.py [--parent-lib PATH] [--out profiles/mixed_classes/bench.json]
    python tools/mixed_bench.py --horizon 15 --batch 16384 --classes 4 --class-pairing --out FILE

One JSON document: every repeat of every leg (ms per step), the leg order, both build ids.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rrt-mpc_amd"))
sys.path.insert(0, str(ROOT / "tests"))


def _bind(path, names):
    """A ctypes handle of the library at `path` with the signatures of mpcqp/_lib.py for `names`."""
    from mpcqp import _lib

    h = ctypes.CDLL(str(path))
    for name in names:
        h_fn = getattr(h, name)
        h_fn.argtypes, h_fn.restype = _lib._SYMBOLS[name]
    return h


class Workspace:
    """One mpcqp workspace with its device inputs and outputs, driven through the C-ABI."""

    def __init__(self, handle, cparams, x0, ref, up, stream, table=None, cls=None, pairing=None, class_pairing=False):
        import torch

        self.h, self.B, self.s = handle, int(x0.shape[0]), ctypes.c_void_p(stream.cuda_stream)
        N = cparams.horizon
        self.ws = ctypes.c_void_p()
        self._check(handle.mpcqp_create(ctypes.byref(cparams), self.B, 0, ctypes.byref(self.ws)), "mpcqp_create")
        dev = torch.device("cuda:0")
        self.x0, self.ref, self.up = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x0, ref, up))
        self.cls = None if cls is None else torch.from_numpy(np.ascontiguousarray(cls, dtype=np.int32)).to(dev)
        self.u0 = torch.empty((self.B, 2), dtype=torch.float64, device=dev)
        self.X = torch.empty((self.B, 4, N + 1), dtype=torch.float64, device=dev)
        self.U = torch.empty((self.B, 2, N), dtype=torch.float64, device=dev)
        self.status = torch.empty((self.B,), dtype=torch.int32, device=dev)
        self.iters = torch.empty((self.B, 4), dtype=torch.int32, device=dev)
        self.active = torch.empty((self.B, 5 * N + 1), dtype=torch.uint8, device=dev)
        if table is not None:
            self._check(handle.mpcqp_set_classes(self.ws, len(table), table), "mpcqp_set_classes")
        if pairing is not None:  # MPCQP_PAIR_*
            self._check(handle.mpcqp_set_pairing(self.ws, pairing), "mpcqp_set_pairing")
        if class_pairing:
            self._check(handle.mpcqp_set_class_pairing(self.ws, 1), "mpcqp_set_class_pairing")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.h.mpcqp_last_error().decode(errors='replace')}")

    def step(self):
        h, ws, B, s = self.h, self.ws, self.B, self.s
        if self.cls is None:
            rc = h.mpcqp_build(ws, B, self.x0.data_ptr(), self.ref.data_ptr(), self.up.data_ptr(), s)
        else:
            rc = h.mpcqp_build_mixed(ws, B, self.x0.data_ptr(), self.ref.data_ptr(), self.up.data_ptr(),
                                     self.cls.data_ptr(), s)
        self._check(rc, "build")
        self._check(h.mpcqp_solve(ws, B, self.u0.data_ptr(), self.X.data_ptr(), self.U.data_ptr(),
                                  self.status.data_ptr(), self.iters.data_ptr(), self.active.data_ptr(), s), "mpcqp_solve")

    def close(self):
        self.h.mpcqp_destroy(self.ws)


def time_leg(workspaces, steps, warmup, stream):
    """ms per step of one step of every workspace in turn, on one stream, by device events."""
    import torch

    for _ in range(warmup):
        for w in workspaces:
            w.step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        for w in workspaces:
            w.step()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", type=Path, default=None,
                    help="libmpcqp.so built from the parent commit (leg plain_parent; skipped when absent)")
    ap.add_argument("--classes", type=int, default=9, help="the first K blocks of tests/param_variants.py VARIANTS")
    ap.add_argument("--class-pairing", action="store_true",
                    help="add the class-paired mixed leg and the K plain launches under MPCQP_PAIR_ON (N <= 15)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mixed_classes" / "bench.json")
    a = ap.parse_args()
    import torch
    from bench_common import interleaved
    from param_variants import VARIANTS, resolution, variant

    from mpcqp import _lib, scenarios
    from mpcqp.config import MPCConfig

    if not torch.cuda.is_available():
        raise SystemExit("mixed_bench needs a GPU (no CPU fallback, no CPU timing)")
    B, N = a.batch, a.horizon
    base_names = ["mpcqp_create", "mpcqp_destroy", "mpcqp_build", "mpcqp_solve", "mpcqp_last_error", "mpcqp_build_id"]
    new = _bind(_lib.LIB_PATH, base_names + ["mpcqp_set_classes", "mpcqp_build_mixed", "mpcqp_set_pairing",
                                             "mpcqp_set_class_pairing", "mpcqp_class_slots", "mpcqp_class_slot_waves",
                                             "mpcqp_launch_info"])
    parent = _bind(a.parent_lib, base_names) if a.parent_lib else None
    batch = scenarios.config3(B, horizon=N)
    base = MPCConfig(horizon=N).to_parameters(0.8)
    if not 2 <= a.classes <= len(VARIANTS):
        raise SystemExit(f"--classes must lie in [2, {len(VARIANTS)}]")
    blocks = [variant(MPCConfig(horizon=N).to_parameters(resolution(v)), v) for v in VARIANTS[:a.classes]]
    K = len(blocks)
    mixed_k, k_plain = f"mixed_k{K}", "nine_plain" if K == 9 else f"{K}_plain"
    cls9 = (np.arange(B) % K).astype(np.int32)
    stream = torch.cuda.current_stream(torch.device("cuda:0"))
    inputs = (batch.x0, batch.ref, batch.u_prev)
    cbase = _lib.to_c_params(base)
    legs = {
        "plain": [Workspace(new, cbase, *inputs, stream)],
        "mixed_k1": [Workspace(new, cbase, *inputs, stream, _lib.class_table([base]), np.zeros(B, np.int32))],
        mixed_k: [Workspace(new, cbase, *inputs, stream, _lib.class_table(blocks), cls9)],
        k_plain: [Workspace(new, _lib.to_c_params(p), *(x[cls9 == c] for x in inputs), stream)
                       for c, p in enumerate(blocks)],
    }
    if parent is not None:
        legs["plain_parent"] = [Workspace(parent, cbase, *inputs, stream)]
    if a.class_pairing:
        legs[mixed_k + "_paired"] = [Workspace(new, cbase, *inputs, stream, _lib.class_table(blocks), cls9,
                                               class_pairing=True)]
        legs[k_plain + "_paired"] = [Workspace(new, _lib.to_c_params(p), *(x[cls9 == c] for x in inputs), stream,
                                               pairing=_lib.PAIRING_MODES["on"]) for c, p in enumerate(blocks)]
    order = [k for k in ("plain", "plain_parent", "mixed_k1", mixed_k, mixed_k + "_paired", k_plain,
                         k_plain + "_paired") if k in legs]
    # the legs alternate: every repeat visits each once, in this order (each timing warms itself up: no repeat 0)
    ms, _ = interleaved({k: lambda k=k: time_leg(legs[k], a.steps, a.warmup, stream) for k in order}, a.repeats,
                        rotate=False, warmup=False)
    torch.cuda.synchronize()
    # what the timed launches computed: the same QPs solved, and the same results where they must be
    solved = {k: int(sum(int((w.status == 1).sum()) for w in legs[k])) for k in order}
    same = {"mixed_k1_equals_plain_bitwise": all(torch.equal(getattr(legs["mixed_k1"][0], f), getattr(legs["plain"][0], f))
                                                 for f in ("u0", "X", "U", "status", "iters", "active"))}
    m9 = legs[mixed_k][0]
    same[f"{mixed_k}_equals_{k_plain}_bitwise"] = all(
        torch.equal(getattr(m9, f)[torch.from_numpy(cls9 == c).to(m9.status.device)], getattr(w, f))
        for c, w in enumerate(legs[k_plain]) for f in ("u0", "X", "U", "status", "iters", "active"))
    launches, slot_us = {}, None
    if a.class_pairing:
        mp = legs[mixed_k + "_paired"][0]
        same[f"{mixed_k}_paired_equals_{mixed_k}_bitwise"] = all(
            torch.equal(getattr(mp, f), getattr(m9, f)) for f in ("u0", "X", "U", "status", "iters", "active"))
        for k in (mixed_k, mixed_k + "_paired", k_plain + "_paired"):  # what ran: QPs per wave, workgroups
            info = (ctypes.c_int32 * 4)()
            new.mpcqp_launch_info(legs[k][0].ws, info)
            launches[k] = {"per_wave": int(info[1]), "workgroups": int(info[2]), "count": int(info[3])}
        # the slot kernel alone, over this batch's classes: device events around `steps` calls, `repeats` times
        slots = torch.empty(2 * new.mpcqp_class_slot_waves(B, K), dtype=torch.int32, device="cuda:0")
        s = ctypes.c_void_p(stream.cuda_stream)
        slot_us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.steps):
                new.mpcqp_class_slots(B, K, mp.cls.data_ptr(), None, slots.data_ptr(), s)
            e1.record(stream)
            e1.synchronize()
            slot_us.append(1e3 * e0.elapsed_time(e1) / a.steps)
    if parent is not None:
        same["plain_equals_parent_bitwise"] = all(
            torch.equal(getattr(legs["plain_parent"][0], f), getattr(legs["plain"][0], f))
            for f in ("u0", "X", "U", "status", "iters", "active"))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {
        "workload": f"config3, B = {B}, N = {N}; {K} classes = the first {K} of tests/param_variants.py VARIANTS, "
                    f"cls[b] = b % {K}",
        "device": torch.cuda.get_device_name(0),
        "timing": f"device events around {a.steps} timed steps after {a.warmup} warm steps; {a.repeats} repeats per "
                  "leg, legs alternating within one process",
        "leg_order": order,
        "build_id": new.mpcqp_build_id().decode(),
        "parent_build_id": parent.mpcqp_build_id().decode() if parent is not None else None,
        "ms_per_step": ms,
        "median_ms_per_step": med,
        "min_max_ms_per_step": {k: [float(min(v)), float(max(v))] for k, v in ms.items()},
        "qp_per_s_median": {k: B / (1e-3 * med[k]) for k in order},
        "solved_qps": solved,
        "results": same,
        "ratio_mixed_k1_to_plain": med["mixed_k1"] / med["plain"],
        f"ratio_{mixed_k}_to_{k_plain}": med[mixed_k] / med[k_plain],
        "ratio_plain_to_parent": med["plain"] / med["plain_parent"] if parent is not None else None,
    }
    if a.class_pairing:
        out["launches"] = launches
        out["slot_kernel_us"] = slot_us
        out["slot_kernel_us_median"] = float(np.median(slot_us))
        out[f"ratio_{mixed_k}_paired_to_{mixed_k}"] = med[mixed_k + "_paired"] / med[mixed_k]
        out[f"ratio_{mixed_k}_paired_to_{k_plain}_paired"] = med[mixed_k + "_paired"] / med[k_plain + "_paired"]
    for ws in legs.values():
        for w in ws:
            w.close()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
