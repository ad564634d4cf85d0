#!/bin/bash
# Per-kernel disassembly of libtristage's gfx950 code: the current tree against a git revision (default HEAD).
# Needs no GPU.  Prints the kernels whose instruction stream differs and the kernels that are new.
#   tools/kernel_disasm_diff.sh [REV [RENAME]]
# RENAME: a sed -E expression applied to the names of REV's kernels before the comparison, so that a renamed kernel is
# compared with its predecessor and not reported as gone and new.  For the commit that made the coalesced scans one
# template per family (scan_{multi,wide}_kernel<DT, G> and scan_{multi,wide}_tomb_kernel<DT, G> became
# scan_{multi,wide}_kernel<DT, G, TOMB>, whose parameter type is spelled in terms of TOMB):
#   tools/kernel_disasm_diff.sh HEAD~ 's/_Z[0-9]+scan_(multi|wide)_(tomb_)?kernel(ILi[0-9]+ELi[0-9]+)EEv[0-9]+[A-Za-z]+Params/\1 \3 Lb0\2/; s/Lb0tomb_/Lb1/; s/multi (.*) (Lb[01])/_Z17scan_multi_kernel\1E\2EEvNSt11conditionalIXT1_E15MultiTombParams15MultiScanParamsE4typeE/; s/wide (.*) (Lb[01])/_Z16scan_wide_kernel\1E\2EEvNSt11conditionalIXT1_E14WideTombParams14WideScanParamsE4typeE/'
# For the commit that made four per-pass scans one template (scan_kernel<DT, QH, MODE>, scan_masked_kernel<DT, QH>,
# scan_fp8_kernel<QH, MODE> and scan_fp8_masked_kernel<QH> became scan_kernel<QH, MODE, OP, WALK>):
#   tools/kernel_disasm_diff.sh HEAD~ 's/_Z11scan_kernelILi([0-9])ELi([0-9])ELi([0-9])EEv10ScanParams/_Z11scan_kernelILi\2ELi\3E4Op16ILi\1EE11WalkStridedEvNT2_6ParamsE/; s/_Z18scan_masked_kernelILi([0-9])ELi([0-9])EEv16MaskedScanParams/_Z11scan_kernelILi\2ELi1E4Op16ILi\1EE8WalkLiveEvNT2_6ParamsE/; s/_Z15scan_fp8_kernelILi([0-9])ELi([0-9])EEv10ScanParams/_Z11scan_kernelILi\1ELi\2E5OpFp811WalkStridedEvNT2_6ParamsE/; s/_Z22scan_fp8_masked_kernelILi([0-9])EEv16MaskedScanParams/_Z11scan_kernelILi\1ELi1E5OpFp88WalkLiveEvNT2_6ParamsE/'
# (a kernel's file holds its instructions and not its name, which is the file's: a renamed kernel can compare equal)
set -e
REV=${1:-HEAD}
RENAME=${2:-}
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
      awk -v d="$2" -v n="$n" '/^<.*>:$/ {s=$1; gsub(/[<>:]/,"",s); f=d"/"n"__"s".fn"; next} f {print > f}'
  done
}
split "$W/base_build" "$W/dis_base"
split "$W/new_build" "$W/dis_new"
same=0; diff=0
for f in "$W"/dis_base/*.fn; do
  b=$(basename "$f")
  [ -z "$RENAME" ] || b=$(printf '%s\n' "$b" | sed -E "$RENAME")
  echo "$b" >> "$W/matched"
  if cmp -s "$f" "$W/dis_new/$b"; then same=$((same + 1)); else diff=$((diff + 1)); echo "CHANGED $b"; fi
done
for f in "$W"/dis_new/*.fn; do grep -qxF "$(basename "$f")" "$W/matched" || echo "NEW $(basename "$f")"; done
echo "kernels of $REV: $same unchanged, $diff changed"
