"""A/B of the super-tile S-pass's two static unit orders over active counts (needs the GPU).

    python scripts/spass_order_sweep.py OUT.json [--dim 4000] [--counts 8,16,32,40,48,53,56,64]

For every count B: one engine of B instances (symmetric tiles, super-tile kernel forced), the HVP
entry (one S-pass launch over all B instances, one right-hand side), timed by the library's own
HIP events.  The order is read at bind (RIPTRM_SUP_BALANCED), so the same engine is rebound
alternately with either order, ROUNDS times; each round times GROUP launches after WARM untimed
ones.  Reports, per count and order, the rounds' us per launch (min / median / max)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "riemannian-interior-point-trust-region-method_amd")]

ROUNDS, GROUP, WARM = 4, 12, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--dim", type=int, default=4000)
    ap.add_argument("--counts", default="8,16,32,40,48,53,56,64")
    a = ap.parse_args()
    import torch
    import engine

    rows = []
    for B in [int(c) for c in a.counts.split(",")]:
        eng = engine.NonnegPCABatch(a.dim, B, log_capacity=16, layout="sym", spass_kind=2, drain_logs=False)
        x0, y0 = eng.generate_synthetic(seed0=777)
        v = torch.randn((B, a.dim), dtype=torch.float64, device=eng.device)
        us = {"balanced": [], "index": []}
        for _ in range(ROUNDS):
            for order, knob in (("index", "0"), ("balanced", "1")):
                os.environ["RIPTRM_SUP_BALANCED"] = knob
                eng.bind()
                for _ in range(WARM):
                    eng.hvp(x0, y0, 0.01, v)
                engine.profile_enable(eng, True)
                for _ in range(GROUP):
                    eng.hvp(x0, y0, 0.01, v)
                p = engine.profile_read(eng)
                engine.profile_enable(eng, False)
                assert p["gemv_launches"] == GROUP, p
                us[order].append(p["gemv_ms"] * 1e3 / GROUP)
        row = {"active": B}
        for order, vals in us.items():
            row[order] = {"min": min(vals), "median": statistics.median(vals), "max": max(vals), "rounds": vals}
        row["balanced_over_index"] = row["balanced"]["median"] / row["index"]["median"]
        rows.append(row)
        print(B, {k: round(row[k]["median"], 1) for k in us}, round(row["balanced_over_index"], 4), flush=True)
        del eng
        torch.cuda.empty_cache()
    os.environ.pop("RIPTRM_SUP_BALANCED", None)
    out = {"what": "k_spass_sup, us per launch through riptrm_nonnegpca_hvp (forced kind 2, one right-hand side), "
                   "unit order read at bind: index (default) vs balanced (RIPTRM_SUP_BALANCED=1)",
           "n": a.dim, "rounds": ROUNDS, "launches_per_round": GROUP, "warmup_launches": WARM, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
