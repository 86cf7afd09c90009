#!/bin/bash
# Kernel-only durations (rocprofv3 --kernel-trace --stats, a run of its own) of the gc_attn kernels: GC_attn(128) forward + backward at
# [32,128,40960] in both layouts, with the streaming kernels' algorithmic bytes (|x|, 2|x|, 2|x|, 3|x|) over their time against 6.3 TB/s.
# usage (GPU box): bash tools/gc_attn_trace.sh > profiles/gc_attn_kernel_stats.txt
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$T" -o r -- python "$R/tools/gc_attn_bench.py" --trace-pass > "$T/run.log" 2>&1 || { tail -20 "$T/run.log"; rm -rf "$T"; exit 1; }
DB=$(find "$T" -name "*.db" | head -1)
python - "$DB" <<'PY'
import re, sqlite3, sys
c = sqlite3.connect(sys.argv[1])
X = 32 * 128 * 40960 * 4
PASSES = {"pool_cm_lds": 1, "bwd_apply_cm_lds": 3, "pool_cm": 1, "pool_pm": 1, "apply_cm": 2, "apply_pm": 2, "bwd_reduce_cm": 2, "bwd_reduce_pm": 2, "bwd_apply_cm": 3, "bwd_apply_pm": 3}
print("# rocprofv3 --kernel-trace --stats: GC_attn(128) forward + backward at [32,128,40960], |x| = %.1f MB, channel-major then point-major rows" % (X / 1e6))
print("%-44s %6s %10s %10s %8s %8s" % ("kernel", "calls", "avg_us", "min_us", "TB/s", "of 6.3"))
rows = c.execute("select name, count(*), avg(duration), min(duration) from kernels group by name order by sum(duration) desc").fetchall()
for n, cnt, av, mn in rows:
    s = re.sub(r"\(anonymous namespace\)::", "", n)
    s = re.sub(r"^void ", "", s)
    s = re.sub(r"\(.*$", "", s)
    key = next((k for k in PASSES if s.startswith(k + "_kernel")), None)
    bw = "" if key is None else "%8.2f %7.0f%%" % (PASSES[key] * X / av * 1e-3, PASSES[key] * X / av * 1e-3 / 6.3 * 100)
    print("%-44s %6d %10.1f %10.1f %s" % (s[:44], cnt, av / 1e3, mn / 1e3, bw))
PY
rm -rf "$T"
