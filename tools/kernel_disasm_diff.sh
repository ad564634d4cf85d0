#!/bin/bash
# Per-kernel disassembly of libtristage's gfx950 code: the current tree against a git revision (default HEAD).
# Needs no GPU.  Prints the kernels whose instruction stream differs and the kernels that are new.
#   tools/kernel_disasm_diff.sh [REV]
set -e
REV=${1:-HEAD}
R=$(cd "$(dirname "$0")/.." && pwd)
W=$(mktemp -d)
trap 'rm -rf "$W"' EXIT
L=/opt/rocm/llvm/bin
mkdir -p "$W/base"
git -C "$R" archive "$REV" tristage-rag_amd/csrc include | tar -x -C "$W/base"
make -s -C "$W/base/tristage-rag_amd/csrc" -j8 OUT="$W/base.so" BUILD="$W/base_build" > /dev/null
make -s -C "$R/tristage-rag_amd/csrc" -j8 OUT="$W/new.so" BUILD="$W/new_build" > /dev/null
split() {  # split <build dir> <out dir>
  mkdir -p "$2"
  for o in "$1"/*.o; do
    n=$(basename "$o" .o)
    $L/llvm-objcopy --dump-section=.hip_fatbin="$2/$n.fb" "$o" /dev/null
    $L/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$2/$n.fb" \
      --output="$2/$n.co" --unbundle
    # (address comments and <symbol+offset> labels move with the code around a kernel: stripped)
    $L/llvm-objdump -d --no-show-raw-insn --no-leading-addr "$2/$n.co" |
      sed -E 's/ *\/\/ [0-9A-F]+:.*$//; s/<[^>]*\+0x[0-9a-f]+>//' |
      awk -v d="$2" -v n="$n" '/^<.*>:$/ {s=$1; gsub(/[<>:]/,"",s); f=d"/"n"__"s".fn"} f {print > f}'
  done
}
split "$W/base_build" "$W/dis_base"
split "$W/new_build" "$W/dis_new"
same=0; diff=0
for f in "$W"/dis_base/*.fn; do
  b=$(basename "$f")
  if cmp -s "$f" "$W/dis_new/$b"; then same=$((same + 1)); else diff=$((diff + 1)); echo "CHANGED $b"; fi
done
for f in "$W"/dis_new/*.fn; do [ -f "$W/dis_base/$(basename "$f")" ] || echo "NEW $(basename "$f")"; done
echo "kernels of $REV: $same unchanged, $diff changed"
