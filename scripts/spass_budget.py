"""Per-launch budget of the S-pass from a rocprofv3 kernel trace of the headline benchmark.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o head -- python bench.py
    python scripts/spass_budget.py DIR/**/head_kernel_trace.csv OUT.json [--bench-json LINE.json] [--tag TAG]

For every S-pass launch (k_spass_sup / k_spass_sym / k_gemv), in start order over both queues:
  dur_us     kernel duration (whole microseconds)
  gap_dus    idle time from its end to the start of the next S-pass on either queue (tenths of a
             microsecond; negative = the two overlapped)
  active     estimated active instances.  The grid says little (a launch of two or more instances
             already has one workgroup per CU), so the estimate is duration / (time per instance),
             the time per instance being the mean duration over the mean instance-passes per launch
             (from the benchmark's own counters when --bench-json is given, else --mean-active)
  boundary   indices of the launches whose gap spans a chunk boundary: the host drained both queues
             and read the list counts back.  Told from the trace alone: a state kernel both started
             and finished inside the gap (at a hand-over inside a chunk the finished pass's state
             kernel, ~40 us, is still running when the other group's pass starts) and the chip
             then stood idle for more than IDLE_US before the next S-pass started
  serial     indices of the launches whose gap holds a whole state kernel but no such idle time:
             the next S-pass belongs to the same group and waited for that state kernel (the
             other group has nothing queued)
The summary holds the histogram of the estimated active counts, the histogram of the hand-over
gaps inside chunks (1 us bins) and the budget per launch.  The per-launch arrays themselves (about
0.6 MB for the headline run) are written only with --per-launch; the committed summaries under
profiles/ leave them out."""
import argparse
import bisect
import csv
import json
import statistics

SPASS = ("k_spass_sup", "k_spass_sym", "k_gemv")
IDLE_US = 10.0


def col(row, *names):
    for k in row:
        if k and k.strip().lower() in names:
            return k
    raise SystemExit(f"no column {names} in {list(row)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("out")
    ap.add_argument("--bench-json", default="", help="the benchmark's result line of the traced run")
    ap.add_argument("--mean-active", type=float, default=0.0, help="mean instance-passes per launch, without --bench-json")
    ap.add_argument("--tag", default="")
    ap.add_argument("--per-launch", action="store_true", help="also write the per-launch arrays")
    a = ap.parse_args()

    sp, st = [], []
    with open(a.trace, newline="") as f:
        rd = csv.DictReader(f)
        kn = ks = ke = kg = None
        for row in rd:
            if kn is None:
                kn, ks, ke = col(row, "kernel_name"), col(row, "start_timestamp"), col(row, "end_timestamp")
                kg = col(row, "grid_size_x", "grid_size")
            name = row[kn]
            if any(s in name for s in SPASS):
                sp.append((int(row[ks]), int(row[ke]), int(row[kg])))
            elif "k_state" in name:
                st.append((int(row[ks]), int(row[ke])))
    sp.sort()
    st.sort()
    if len(sp) < 2:
        raise SystemExit("no S-pass launches in the trace")
    st_start = [s for s, _ in st]

    n = len(sp)
    dur = [(e - s) / 1e3 for s, e, _ in sp]
    gap = [(sp[i + 1][0] - sp[i][1]) / 1e3 for i in range(n - 1)]
    boundary, serial = [], []
    for i in range(n - 1):
        lo, hi = sp[i][1], sp[i + 1][0]
        j = bisect.bisect_left(st_start, lo)
        last_end = None
        while j < len(st) and st[j][0] < hi:
            if st[j][1] <= hi:
                last_end = st[j][1] if last_end is None else max(last_end, st[j][1])
            j += 1
        if last_end is not None:
            (boundary if (hi - last_end) / 1e3 > IDLE_US else serial).append(i)
    bset, sset = set(boundary), set(serial)

    mean_active, src = a.mean_active, "--mean-active"
    if a.bench_json:
        line = json.loads(open(a.bench_json).read().strip().splitlines()[-1])
        d = line["detail"]
        # instance-passes and launches of the timed window
        mean_active = d["s_passes_per_s"] * (line["ms_per_step"] * line["steps"] / 1e3) / d["gemv_launches"]
        src = "the traced run's s_passes_per_s x window / gemv_launches"
    per_inst = statistics.fmean(dur) / mean_active if mean_active > 0 else 0.0
    active = [max(1, round(x / per_inst)) if per_inst > 0 else 0 for x in dur]
    hist = {}
    for v in active:
        hist[v] = hist.get(v, 0) + 1

    inner = [g for i, g in enumerate(gap) if i not in bset and i not in sset]
    ghist = {}
    for g in inner:
        b = max(-1, min(60, int(g // 1)))   # -1: overlapped, 60: 60 us or more
        ghist[b] = ghist.get(b, 0) + 1
    outer = [g for i, g in enumerate(gap) if i in bset]
    ser = [g for i, g in enumerate(gap) if i in sset]
    span = (sp[-1][1] - sp[0][0]) / 1e3
    out = {
        "tag": a.tag,
        "source": "rocprofv3 --kernel-trace --stats of the default bench.py command (whole process: warm-up and timed window)",
        "units": {"dur_us": "us", "gap_dus": "0.1 us", "active": "instances (estimated from the duration)"},
        "summary": {
            "launches": n,
            "mean_dur_us": statistics.fmean(dur),
            "mean_active_assumed": mean_active, "mean_active_source": src, "us_per_instance": per_inst,
            "hand_overs_inside_chunks": len(inner),
            "mean_gap_inside_chunk_us": statistics.fmean(inner) if inner else None,
            "median_gap_inside_chunk_us": statistics.median(inner) if inner else None,
            "chunk_boundaries": len(outer),
            "mean_gap_at_chunk_boundary_us": statistics.fmean(outer) if outer else None,
            "median_gap_at_chunk_boundary_us": statistics.median(outer) if outer else None,
            "same_group_hand_overs": len(ser),
            "mean_gap_same_group_us": statistics.fmean(ser) if ser else None,
            "per_launch_us": {
                "kernel": statistics.fmean(dur),
                "idle_inside_chunks": sum(inner) / n,
                "idle_at_chunk_boundaries": sum(outer) / n,
                "idle_at_same_group_hand_overs": sum(ser) / n,
                "first_start_to_last_end": span / n,
            },
            "spass_busy_frac": sum(dur) / span,
            "active_histogram": {str(k): hist[k] for k in sorted(hist)},
            "gap_inside_chunk_histogram_us": {str(k): ghist[k] for k in sorted(ghist)},
        },
    }
    if a.per_launch:
        out["launch"] = {
            "dur_us": [round(x) for x in dur],
            "gap_dus": [round(10 * g) for g in gap] + [0],
            "active": active,
            "grid_threads_distinct": sorted({g for _, _, g in sp}),
            "boundary": boundary,
            "serial": serial,
        }
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":")) if a.per_launch else json.dump(out, f, indent=1)
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
