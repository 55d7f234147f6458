#!/bin/bash
# Register / spill / LDS report of the kernels of one translation unit (cross-compiles, no GPU needed):
#   tools/regs.sh [UNIT [PATTERN]]
# UNIT is a csrc/*.hip without its suffix (default cheb_struct), compiled with the flags csrc/Makefile gives that unit plus $EXTRA;
# PATTERN is a regex on the (demangled) kernel signature (default: every kernel).  One line per kernel, sorted by signature:
#   SGPR VGPR AGPR scratch[B/lane] waves/SIMD SGPR-spill VGPR-spill LDS[B/block]  signature
# e.g. `tools/regs.sh dense_attention_split dq_kernel`; to compare two commits, diff the two outputs.
unit=${1:-cheb_struct}
pattern=${2:-.}
csrc="$(cd "$(dirname "$0")/../deepsphere-cosmo-tf2_amd/csrc" && pwd)" || exit 1
[ -f "$csrc/$unit.hip" ] || { echo "regs.sh: no $csrc/$unit.hip" >&2; exit 1; }
out="$(mktemp -d)" || exit 1
trap 'rm -rf "$out"' EXIT
# the unit's compile line as make would run it, with the object sent elsewhere
cmd="$(make -C "$csrc" -n -B "$csrc/build/$unit.o" | grep -e "-c $csrc/$unit\.hip" | head -1)"
[ -n "$cmd" ] || { echo "regs.sh: csrc/Makefile has no rule for build/$unit.o" >&2; exit 1; }
demangle=cat
command -v c++filt > /dev/null && demangle=c++filt
${cmd% -o *} $EXTRA -o "$out/$unit.o" -Rpass-analysis=kernel-resource-usage -fno-caret-diagnostics 2>&1 | sed 's/ *\[-Rpass[^]]*\]//' | awk '
  /(error|warning):/ { print > "/dev/stderr" }
  /Function Name:/ { name = $NF }
  /remark:.* (TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes\/lane\]|Occupancy \[waves\/SIMD\]|SGPRs Spill|VGPRs Spill): [0-9]+$/ { row = row " " $NF }
  /LDS Size \[bytes\/block\]:/ { print substr(row, 2) " " $NF "  " name; row = "" }' | $demangle | grep -E "$pattern" | sort -k9
