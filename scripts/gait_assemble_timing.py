"""HIP-event timings of the on-device controller-QP assembly: qpb_assemble_gait for one
stance mask of each phase next to qpb_assemble_controller (the stance kernel, the
yardstick) in the same run, B QPs each (default 8 192, one tick's candidates).

    python scripts/gait_assemble_timing.py [--B 8192] [--reps 200] [--rounds 9] [--out FILE]

Every round times `reps` back-to-back launches of each case between two events, the
cases interleaved; reported: the median over rounds of the time per launch, the
case's table entries (one per position of P's stored triangle, A and G plus the rows
of c, h, b) and the time per entry per QP.  `check` is not passed, so a call is the
assembly kernel alone.  One JSON line per case, a summary line last."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from apf_quadruped_amd import workloads as W  # noqa: E402
from apf_quadruped_amd.batch import Plan, to_tiled  # noqa: E402

SEED = 0xD06B07 + 62


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--masks", default="0xA,0x5,0xE,0x7", help="stance masks timed through qpb_assemble_gait")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    B = a.B
    cases = []
    for name, stance in [("assemble_controller", None)] + [(f"assemble_gait {m}", int(m, 16)) for m in a.masks.split(",")]:
        t = W.controller_gait_terms(SEED, np.arange(B), 0xF if stance is None else stance)
        d = W.controller_gait_qp_from_terms({k: v[:1] for k, v in t.items()}, 0xF if stance is None else stance)
        plan = Plan.from_dense(30, d["m"], d["p"], d["P"][0], d["A"][0], d["G"][0])
        terms = torch.from_numpy(to_tiled(W.pack_terms(t))).cuda()
        swing = torch.from_numpy(to_tiled(W.pack_swing(t))).cuda()
        if stance is None:
            out = plan.assemble_controller(terms, B=B)
            call = (lambda plan=plan, terms=terms, out=out: plan.assemble_controller(terms, B=B, out=out))
        else:
            out = plan.assemble_gait(terms, stance, swing=swing, B=B)
            call = (lambda plan=plan, terms=terms, swing=swing, out=out, stance=stance:
                    plan.assemble_gait(terms, stance, swing=swing, B=B, out=out))
        entries = 465 + 30 * d["p"] + 30 * d["m"] + 30 + d["m"] + d["p"]
        stored = plan.info.nnzP + plan.info.nnzA + plan.info.nnzG + 30 + d["m"] + d["p"]
        cases.append(dict(name=name, shape=[30, d["m"], d["p"]], entries=entries, stored=stored, call=call, ms=[]))
    for c in cases:                                   # warm-up: table upload, code object
        for _ in range(20):
            c["call"]()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for c in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                c["call"]()
            e1.record()
            e1.synchronize()
            c["ms"].append(e0.elapsed_time(e1) / a.reps)
    lines = []
    for c in cases:
        med = float(np.median(c["ms"]))
        lines.append(dict(case=c["name"], B=B, shape=c["shape"], table_entries=c["entries"], stored_values=c["stored"],
                          median_us=round(1e3 * med, 3), min_us=round(1e3 * min(c["ms"]), 3),
                          max_us=round(1e3 * max(c["ms"]), 3),
                          ps_per_entry_per_qp=round(1e9 * med / (c["entries"] * B), 3),
                          store_GBps=round(8.0 * c["stored"] * B / (med * 1e-3) / 1e9, 1)))
    base = lines[0]["ps_per_entry_per_qp"]
    lines.append(dict(summary="time per table entry relative to assemble_controller",
                      ratio={ln["case"]: round(ln["ps_per_entry_per_qp"] / base, 3) for ln in lines[1:]},
                      reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0)))
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
