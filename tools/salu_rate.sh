#!/usr/bin/env bash
# Runs tools/salu_rate (built by: hipcc --offload-arch=gfx950 -O2 -o tools/salu_rate tools/salu_rate.hip) for every mix at 1, 2,
# 4, 8 and 16 waves per CU (one wave alone, one per SIMD on 2 and 4 SIMDs, 2 and 4 per SIMD); every launch is a process of its own under its own time limit, and the first
# one that fails or runs out of time ends the script.
set -uo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
[[ -x "$here/salu_rate" ]] || { echo "build tools/salu_rate first (see the head of this script)"; exit 1; }
for mix in valu salu both salu2 nop branch; do
  for w in 1 2 4 8 16; do
    timeout -k 5 30 "$here/salu_rate" $mix $w || { echo "salu_rate $mix $w: exit $?"; exit 1; }
  done
done
