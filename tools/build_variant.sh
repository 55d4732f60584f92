#!/bin/bash
# One library variant for A/B runs: tools/build_variant.sh <out.so> <source.hip> <extra -D flags...>   (the other objects come
# from the last regular build in diffsptk_amd/lib/obj; the flags are the regular build's: _lib.HIPCC_FLAGS + SOURCE_FLAGS)
OUT=$1; SRC=$2; shift 2
FL=$(python -c "import sys; from diffsptk_amd import _lib; print(*_lib.HIPCC_FLAGS, *_lib.SOURCE_FLAGS.get(sys.argv[1], ()))" "$SRC") || exit 1
mkdir -p build
hipcc $FL "$@" -c diffsptk_amd/csrc/$SRC -o build/variant_$(basename $OUT).o 2>/dev/null || exit 1
OBJS=""
for o in diffsptk_amd/lib/obj/*.o; do
  [ "$(basename $o)" = "$SRC.o" ] && OBJS="$OBJS build/variant_$(basename $OUT).o" || OBJS="$OBJS $o"
done
hipcc --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden -o $OUT $OBJS 2>/dev/null && echo built $OUT
