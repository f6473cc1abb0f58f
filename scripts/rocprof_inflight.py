#!/usr/bin/env python
"""Launches in flight and the gaps between the MSV tier launches of a rocprofv3 kernel trace (rocpd sqlite), over the
trace after its first <skip> fraction (calibration, residency pass): time-weighted mean number of kernels running, share of
the time with 0 / 1 / 2 / 3+ of them, and the stretches with no msv_tier_kernel running (the launch that is 72 % of the
search: a gap is time another cascade's tier launch could have started in).
usage: rocprof_inflight.py <results.db> [skip_first_fraction]"""
import sqlite3
import sys

c = sqlite3.connect(sys.argv[1])
skip = float(sys.argv[2]) if len(sys.argv) > 2 else 0.0
rows = list(c.execute("select name, start, end from kernels order by start"))
t_first, t_last = rows[0][1], max(r[2] for r in rows)
cut = t_first + skip * (t_last - t_first)
rows = [r for r in rows if r[1] >= cut]
t0, t1 = rows[0][1], max(r[2] for r in rows)
span = float(t1 - t0)
ev = sorted([(r[1], 1) for r in rows] + [(r[2], -1) for r in rows])
depth, last, at = 0, t0, [0.0, 0.0, 0.0, 0.0]
weighted = 0.0
for t, d in ev:
    at[min(depth, 3)] += t - last
    weighted += depth * (t - last)
    depth += d; last = t
print(f"{len(rows)} launches over {span / 1e6:.1f} ms: mean launches in flight {weighted / span:.2f}; "
      f"time with 0 / 1 / 2 / 3+ in flight: {100 * at[0] / span:.1f} / {100 * at[1] / span:.1f} / {100 * at[2] / span:.1f} / {100 * at[3] / span:.1f} %")
tiers = sorted((r[1], r[2]) for r in rows if "msv_tier_kernel" in r[0])
if tiers:
    gaps, end = [], tiers[0][1]
    for s, e in tiers[1:]:
        if s > end:
            gaps.append(s - end)
        end = max(end, e)
    tspan = float(end - tiers[0][0])
    gaps.sort()
    tot = float(sum(gaps))
    pick = lambda q: gaps[min(len(gaps) - 1, int(q * len(gaps)))] / 1e6 if gaps else 0.0
    print(f"{len(tiers)} msv_tier launches, {sum(e - s for s, e in tiers) / 1e6:.1f} ms of them over {tspan / 1e6:.1f} ms: no tier launch running for "
          f"{tot / 1e6:.1f} ms ({100 * tot / tspan:.1f} %) in {len(gaps)} gaps, median {pick(0.5):.3f} ms, 90th percentile {pick(0.9):.3f} ms, "
          f"longest {gaps[-1] / 1e6 if gaps else 0.0:.3f} ms; gaps over 1 ms: {sum(1 for g in gaps if g > 1e6)} ({sum(g for g in gaps if g > 1e6) / 1e6:.1f} ms)")
