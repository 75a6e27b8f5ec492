"""Developer tool: per-bounce durations of k_extend / k_shadow / k_shade from a rocprofv3 --kernel-trace CSV of frames rendered with the
passes on one stream: a launch's bounce is its position among the launches of the same kernel family since the last k_raygen.
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 tools/profile_frame.py --config c4 --serial ; python tools/trace_bounces.py DIR 2
(FRAMES, the last argument: the frames the program rendered — profile_frame.py renders a warm-up frame and one more — to print ms per frame)"""
import csv, glob, os, sys, collections
files = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True)
frames = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
rows = []
for f in files:
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", "")))
rows.sort()
tot = collections.defaultdict(float)
per = collections.defaultdict(lambda: collections.defaultdict(lambda: [0.0, 0]))
seen = collections.defaultdict(int)
for s, e, k in rows:
    fam = k.split("<")[0]
    tot[k] += (e - s) / 1e6
    if fam == "k_raygen":
        seen.clear()
        continue
    if fam in ("k_extend", "k_shadow", "k_shade"):
        b = seen[fam]
        seen[fam] += 1
        c = per[fam][(b, k)]
        c[0] += (e - s) / 1e6
        c[1] += 1
print("frames %g; ms per frame by kernel:" % frames)
for k, v in sorted(tot.items(), key=lambda kv: -kv[1])[:14]:
    print("  %-44s %9.2f" % (k[:44], v / frames))
for fam in ("k_extend", "k_shadow", "k_shade"):
    total = sum(c[0] for c in per[fam].values())
    print("%s per bounce (ms per frame, share of the family, launches):" % fam)
    for (b, k), c in sorted(per[fam].items()):
        print("  bounce %d  %-40s %9.2f  %5.1f %%  %d" % (b, k[:40], c[0] / frames, 100.0 * c[0] / max(total, 1e-9), c[1]))
