#!/bin/bash
# build_variant.sh <tag> <extra -D flags...>: a diagnostic build of libmovba into build/libmovba_<tag>.so, from the sources
# and with the flags of mov-slam_amd/csrc/Makefile (every object compiled afresh: the flags differ from call to call)
set -e
TAG=$1; shift
ROOT=$(cd $(dirname $0)/.. && pwd)
B=/tmp/movba_variant_$TAG; mkdir -p $B $ROOT/build
make -C $ROOT/mov-slam_amd/csrc -s -B -j8 lib OUT=$ROOT/build/libmovba_$TAG.so OBJDIR=$B EXTRA="$*"
echo built $ROOT/build/libmovba_$TAG.so
