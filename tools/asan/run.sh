#!/bin/bash
# Host-code AddressSanitizer + UBSan run (CPU only, no GPU needed): rebuilds the host translation units
# with the sanitizers (the device objects' host stubs are linked as built by `make`), runs
# host_asan.cpp over the host entry points, and fails on any sanitizer report.
set -eu
cd "$(dirname "$0")/../.."
make -s all
OUT=ray-tracing-project_amd/build/asan
mkdir -p $OUT
HIPCC=/opt/rocm/bin/hipcc
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined"
FLAGS="-O1 -g -std=c++17 -ffp-contract=off -Iinclude -Iray-tracing-project_amd/csrc"
CSRC=ray-tracing-project_amd/csrc
OBJS=
for src in $CSRC/*.cpp; do  # every host source the Makefile links (rt_version.cpp only embeds the source hash)
  f=$(basename $src .cpp)
  [ $f = rt_version ] && continue
  $HIPCC $FLAGS $SAN -fno-gpu-sanitize -c $src -o $OUT/$f.o
  OBJS="$OBJS $OUT/$f.o"
done
for src in $CSRC/*.hip; do  # every device source the Makefile links (rt_variants.hip is the A/B library's)
  f=$(basename $src .hip)
  [ $f = rt_variants ] && continue
  OBJS="$OBJS ray-tracing-project_amd/build/$f.o"
done
$HIPCC $FLAGS $SAN -fno-gpu-sanitize -c tools/asan/host_asan.cpp -o $OUT/host_asan.o
$HIPCC $SAN -fno-gpu-sanitize --offload-arch=gfx950 -o $OUT/host_asan $OUT/host_asan.o $OBJS -lpthread
ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 $OUT/host_asan scenes
