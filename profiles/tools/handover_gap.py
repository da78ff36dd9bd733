#!/usr/bin/env python3
"""From a rocprofv3 --kernel-trace CSV of a bench run: for every hand-over kernel (k_publish_final) of the ADMM part, the time from its
end to the start of the k_front_cw that follows it (negative: the front started before the hand-over had ended).  With LORADS_SPEC_FRONT the front sits behind the hand-over on the stream, so the gap is
a launch boundary; without it -- and in bench.py's roofline passes, whose timing windows keep every front where it was -- the gap holds
the flag's way to the host, the caller's decisions and the next enqueue.  The pairs are therefore reported in two classes: gap below
2 us (back to back) and the rest.
usage: handover_gap.py trace.csv"""
import csv
import statistics
import sys

rows = [r for r in csv.DictReader(open(sys.argv[1]))]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
last = max(i for i, r in enumerate(rows) if any(k in r["Kernel_Name"] for k in ("k_his_two", "k_lbfgs_team", "k_alm_close")))
adm = rows[last + 1:]
gaps = []
for i, r in enumerate(adm):
    if "k_publish_final" not in r["Kernel_Name"]:
        continue
    nxt = next((q for q in adm[i + 1:i + 4] if "k_front_cw" in q["Kernel_Name"]), None)
    if nxt is not None:
        gaps.append((int(nxt["Start_Timestamp"]) - int(r["End_Timestamp"])) / 1e3)
if not gaps:
    sys.exit("no k_publish_final followed by k_front_cw in the ADMM part")
gaps.sort()
for label, g in (("back to back (< 2 us)", [x for x in gaps if x < 2.0]), ("host in between (>= 2 us)", [x for x in gaps if x >= 2.0])):
    if g:
        print("%-26s %4d pairs  median %6.2f us  min %6.2f  max %7.2f" % (label, len(g), statistics.median(g), g[0], g[-1]))
    else:
        print("%-26s    0 pairs" % label)
print("hand-over end -> next k_front_cw start: %d pairs  median %.2f us  mean %.2f us  min %.2f  p90 %.2f  max %.2f" %
      (len(gaps), statistics.median(gaps), sum(gaps) / len(gaps), gaps[0], gaps[int(0.9 * (len(gaps) - 1))], gaps[-1]))
