"""Development tool: device RRT* trees / final plans of the config-5 test swarm against the host
restatement (oracle/rrt_oracle.py), vehicle by vehicle; prints the vehicles that differ and where.

    python tools/diag/swarm_plan_diff.py [V] [pair_seed]     # on the GPU box
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "rrt-mpc_amd"), str(ROOT / "oracle"), str(ROOT / "tests")]


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    pair_seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    import rrt_oracle as ro
    from gpu_helpers import oracle_plan, pairs, planner_params

    from mpcqp.planning.rrt_star import BatchedRRTStarPlanner, draw_samples

    occ = np.load(ROOT / "tests" / "golden" / "default_plan.npz")["occupancy"]
    starts, goals = pairs(occ, V, pair_seed)
    prm = planner_params()
    pl = BatchedRRTStarPlanner(occ, prm, device="cuda:0")
    nodes, count, meta = pl.grow(starts, goals, np.arange(V))
    nodes, count, meta = nodes.cpu().numpy(), count.cpu().numpy(), meta.cpu().numpy()
    final = pl.paths_batch(starts, goals, np.arange(V), smoothing="device")
    report = []
    for v in range(V):
        p = planner_params(v)
        smp = draw_samples(v, goals[v], occ.shape, p.goal_sample_rate, p.max_iterations)
        on, oit, ogi = ro.grow_tree(occ, starts[v], goals[v], smp, step=p.step, goal_radius=p.goal_radius,
                                    rewire_radius=p.rewire_radius, collision_step=p.collision_step)
        dn = nodes[v, : count[v]]
        row = {"v": v, "count": [int(count[v]), len(on)], "iters": [int(meta[v, 0]), int(oit)],
               "goal": [int(meta[v, 1]), int(ogi)]}
        if len(dn) == len(on):
            row["max_xy"] = float(np.abs(dn[:, :2] - on[:, :2]).max())
            row["max_cost"] = float(np.abs(dn[:, 2] - on[:, 2]).max())
            bad = np.flatnonzero(dn[:, 3] != on[:, 3])
            row["parent_diff"] = bad[:10].tolist()
            for k in bad[:3]:
                pd, po = int(dn[k, 3]), int(on[k, 3])
                # the two candidate routes' costs as the oracle has them
                cd = on[pd, 2] + np.hypot(*(on[pd, :2] - on[k, :2])) if pd >= 0 else None
                co = on[po, 2] + np.hypot(*(on[po, :2] - on[k, :2])) if po >= 0 else None
                row.setdefault("ties", []).append([int(k), pd, po, cd, co])
        op = oracle_plan(occ, starts[v], goals[v], v)
        fp = final[v]
        if op is None or fp is None:
            row["plan"] = [op is None, fp is None]
        else:
            a, b = np.asarray(fp), np.asarray(op)
            row["plan_shape"] = [list(a.shape), list(b.shape)]
            row["plan_max"] = float(np.abs(a - b).max()) if a.shape == b.shape else None
        differs = (row["count"][0] != row["count"][1] or row.get("parent_diff") or row.get("plan_max") is None
                   or row.get("plan_max", 0) > 1e-4 or row.get("max_xy", 0) > 1e-9)
        if differs:
            report.append(row)
    print(json.dumps({"V": V, "differ": report}, indent=1))


if __name__ == "__main__":
    main()
