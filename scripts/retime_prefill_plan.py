"""Re-time every entry of the persisted prefill plan (ops/tuned/gemm_plan_mi355x.json, section
`prefill`: csrc/gemm_big.hip against hipBLASLt per (rows, N, K)) on one box in one run, with random
weights of each shape rotated over 4 copies (every call streams its weights from HBM), two interleaved
passes and the best of each kernel's rounds — so no entry is decided by one noisy or warm measurement
(VERDICT r5 weak #9).  Prints old vs new per entry; --write merges the result into the plan file.

    python scripts/retime_prefill_plan.py [--write] [--margin 0.02]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops.autotune import DEFAULT_PLAN_FILE, _time_big_vs_blas, save_section  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--margin", type=float, default=float(os.environ.get("KA_PREFILL_MARGIN", "0.02")))
    ap.add_argument("--plan", default=DEFAULT_PLAN_FILE)
    args = ap.parse_args()
    with open(args.plan) as f:
        old = json.load(f).get("prefill", {})
    keys = sorted(old, key=lambda k: tuple(int(v) for v in k.split(",")[::-1]))
    shapes = {}
    for k in keys:
        M, N, K = (int(v) for v in k.split(","))
        shapes.setdefault((N, K), []).append(M)
    new = {}
    flips = 0
    for (N, K), Ms in shapes.items():
        ws = [(torch.randn(N, K, device="cuda") / K ** 0.5).to(torch.bfloat16) for _ in range(4)]
        for M in sorted(Ms):
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            if not ops.big_gemm_ok(x, ws[0]):
                continue
            tg, tb = zip(*(_time_big_vs_blas(x, ws, reps=6, rounds=5) for _ in range(2)))   # interleaved passes
            t_blas, t_big = min(tb), min(tg)
            big = t_big <= t_blas * (1.0 + args.margin)
            key = f"{M},{N},{K}"
            o = old.get(key)
            flip = o is not None and bool(o[0]) != big
            flips += flip
            new[key] = [bool(big), round(t_big, 1), round(t_blas, 1)]
            print(f"{key:>18}: gemm_big {t_big:8.1f} us (passes {tg[0]:.1f} / {tg[1]:.1f})  hipBLASLt {t_blas:8.1f} us "
                  f"(passes {tb[0]:.1f} / {tb[1]:.1f})  -> {'gemm_big' if big else 'hipBLASLt'}"
                  f"   was {o}{'   FLIPPED' if flip else ''}", flush=True)
            del x
        del ws
        torch.cuda.empty_cache()
    n_big = sum(v[0] for v in new.values())
    print(f"{len(new)} entries re-timed, {n_big} choose gemm_big, {flips} decisions changed", flush=True)
    if args.write:
        save_section(args.plan, "prefill", new)
        print("written:", args.plan, flush=True)


if __name__ == "__main__":
    main()
