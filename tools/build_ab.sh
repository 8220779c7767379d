#!/bin/bash
# Build a timing variant of the whole library into tools/bin/lib_<tag>.so
# (A/B of two builds in one GPU session via SAMNERF_LIB): usage
#   bash tools/build_ab.sh TAG [-DMACRO ...]     (run from the repo root)
set -e
TAG=$1; shift
OUT=tools/bin/obj_$TAG
mkdir -p $OUT
SRC=segment-anything-nerf_amd/csrc
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -I include $*"
pids=()
# the one source list: build.py's
for f in $(cd segment-anything-nerf_amd && python -c "import build; print(*build.SOURCES)"); do
  if [ "${f##*.}" = cpp ]; then X="-x hip"; else X=""; fi
  hipcc $X $FLAGS -c $SRC/$f -o $OUT/$f.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o tools/bin/lib_$TAG.so $OUT/*.o
rm -rf $OUT
echo tools/bin/lib_$TAG.so
