#!/bin/bash
# The device-only assembly of every translation unit in both builds (default, and parity = -DPDMP_EXTRA_KERNELS) with the library's flags, one
# <outdir>/<build>/<unit>.s each, without the __hip_cuid_<hash of the source> lines.  A refactor that must not change the device code is proved
# by running this on both commits and comparing:
#   tools/isa_compare.sh <outdir> [<outdir of the other commit>]      (hipcc only: runs without a GPU; JOBS=8 compilations at a time)
OUT=${1:?usage: isa_compare.sh outdir [other_outdir]}; OTHER=$2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
UNITS=$(python3 -c "import sys; sys.path.insert(0, '$ROOT/zigzagboomerang.jl_amd'); import build; print(' '.join(build.SOURCES + build.EXTRA_SOURCES))") || exit 1
mkdir -p $OUT/default $OUT/parity || exit 1
one() {  # <build> <unit>
  local DEF=; [ $1 = parity ] && DEF=-DPDMP_EXTRA_KERNELS
  ${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fPIC $DEF -I$ROOT/include --cuda-device-only -S \
    $ROOT/zigzagboomerang.jl_amd/csrc/$2 -o - | grep -v __hip_cuid_ > $OUT/$1/${2%.hip}.s; [ ${PIPESTATUS[0]} = 0 ] || { echo "FAILED $1 $2"; return 1; }
}
export -f one; export OUT ROOT HIPCC
for B in default parity; do for U in $UNITS; do echo $B $U; done; done | xargs -P ${JOBS:-8} -L 1 bash -c 'one $0 $1' || exit 1
for B in default parity; do for U in $UNITS; do
  F=$B/${U%.hip}.s
  [ -z "$OTHER" ] && echo "$F $(wc -l < $OUT/$F) lines" && continue
  cmp -s $OUT/$F $OTHER/$F && echo "$F $(wc -l < $OUT/$F) lines identical" || { echo "$F DIFFERS"; BAD=1; }
done; done
exit ${BAD:-0}
