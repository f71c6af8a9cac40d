#!/bin/bash
# Build a second copy of libssnode.so with extra compiler flags into tools/ab/<tag>/ for A/B timing on ONE box:
#   tools/ab_build.sh kv8 -DSSN_TILE_KV=8     then   SSN_LIBDIR=tools/ab/kv8 python bench.py ...
# Every file is compiled by tc_gan_amd/csrc/Makefile, with its flags for that file, and the extra ones behind them.
set -e
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/ab/$tag
mkdir -p $out/obj
make -C $root/tc_gan_amd/csrc -j4 OBJDIR=$out/obj OUT=$out/libssnode.so LINKMAP= EXTRA="$*"
rm -rf $out/obj
echo built $out/libssnode.so
