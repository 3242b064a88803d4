#!/bin/sh
# Is the gfx950 device code of two builds the same?  For each object named
# (default: the three 3x3-conv TUs) the code object is unbundled from the fat
# binary of DIR_A/NAME.o and of DIR_B/NAME.o, and .text, .rodata and .note are
# compared byte for byte (.note holds the kernels' signatures and resource
# use).  Host-only edits leave all three the same.
#   tools/device_code_cmp.sh DIR_A DIR_B [NAME ...]
set -eu
A=$1; B=$2; shift 2
[ $# -gt 0 ] || set -- conv3x3 conv3x3_u8 convs36
BIN=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
rc=0
for n; do
  for side in A B; do
    eval dir=\$$side
    "$BIN/llvm-objcopy" -O binary --only-section=.hip_fatbin "$dir/$n.o" "$T/$n.$side.fb"
    "$BIN/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
        --input="$T/$n.$side.fb" --output="$T/$n.$side.elf"
    for s in text rodata note; do
      "$BIN/llvm-objcopy" -O binary --only-section=.$s "$T/$n.$side.elf" "$T/$n.$side.$s"
    done
  done
  for s in text rodata note; do
    if cmp -s "$T/$n.A.$s" "$T/$n.B.$s"; then r=same; else r=DIFFERENT; rc=1; fi
    echo "$n .$s $(wc -c < "$T/$n.A.$s") bytes: $r"
  done
done
exit $rc
