#!/bin/bash
# Which compiled kernel instantiations of libtristage a pytest selection launches.
#   tools/kernel_coverage.sh OUT_DIR [pytest arguments ...]        (default selection: tests -m gpu)
# 1. lists the kernel symbols of the gfx950 code objects of the current build (split per object file as in
#    tools/kernel_disasm_diff.sh; no GPU needed),
# 2. runs the selection ONCE under `rocprofv3 --kernel-trace --stats`, under a time limit (COVERAGE_TIMEOUT seconds,
#    default 1500),
# 3. writes OUT_DIR/coverage.txt: per source file, launched / compiled, then every instantiation never launched
#    (and keeps the profiler's kernel statistics as OUT_DIR/kernel_stats.csv; its traces stay in a temporary directory).
# Exit status: that of the profiled pytest run (coverage.txt is written either way when the profiler left its stats).
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:?usage: tools/kernel_coverage.sh OUT_DIR [pytest args]}
shift
[ $# -gt 0 ] || set -- tests -m gpu
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
L=/opt/rocm/llvm/bin
FILT=$L/llvm-cxxfilt
[ -x "$FILT" ] || FILT=c++filt
W=$(mktemp -d)
trap 'rm -rf "$W"' EXIT
make -s -j8 -C "$R/tristage-rag_amd/csrc" > /dev/null || exit 1
: > "$OUT/compiled.txt"
for o in "$R"/tristage-rag_amd/csrc/_build/*.o; do
  n=$(basename "$o" .o)
  $L/llvm-objcopy --dump-section=.hip_fatbin="$W/$n.fb" "$o" /dev/null || exit 1
  $L/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$W/$n.fb" --output="$W/$n.co" \
    --unbundle || exit 1
  # kernels are the symbols with a kernel descriptor (<name>.kd)
  $L/llvm-readelf -s --wide "$W/$n.co" | awk '$NF ~ /\.kd$/ {print substr($NF, 1, length($NF) - 3)}' | sort -u |
    "$FILT" | sed "s/^/$n\t/" >> "$OUT/compiled.txt"
done
(cd "$R" && timeout -k 10 "${COVERAGE_TIMEOUT:-1500}" /opt/rocm/bin/rocprofv3 --kernel-trace --stats -d "$W/prof" -o cov \
  --output-format csv -- python -m pytest "$@" -q -p no:cacheprovider) > "$OUT/pytest.log" 2>&1
rc=$?
tail -3 "$OUT/pytest.log"
stats=$(find "$W/prof" -name '*kernel_stats.csv' | head -1)
if [ -z "$stats" ]; then echo "no kernel statistics from the profiler (exit status $rc)"; exit $(( rc ? rc : 1 )); fi
cp "$stats" "$OUT/kernel_stats.csv"
python3 - "$OUT/compiled.txt" "$OUT/kernel_stats.csv" "$OUT/coverage.txt" "$*" <<'EOF'
import csv, sys
from collections import defaultdict
compiled, stats, out, sel = sys.argv[1:5]
norm = lambda s: "".join(s.split())
launched = {norm(r["Name"]) for r in csv.DictReader(open(stats))}
per = defaultdict(list)
for line in open(compiled):
    obj, name = line.rstrip("\n").split("\t", 1)
    per[obj].append((name, norm(name) in launched))
with open(out, "w") as f:
    f.write(f"kernel instantiations of libtristage (gfx950) launched by: pytest {sel}\n\n")
    for obj in sorted(per):
        f.write(f"{obj}: {sum(l for _, l in per[obj])} of {len(per[obj])} launched\n")
    f.write("\nnever launched:\n")
    for obj in sorted(per):
        for name, l in per[obj]:
            if not l:
                f.write(f"  {obj}  {name}\n")
print(open(out).read())
EOF
exit $rc
