#!/bin/bash
# A/B builds of libcadrays_hip.so with extra -D flags:  tools/ab_build.sh NAME "-DCRH_X=1 ..." [NAME2 "flags2" ...]
# Outputs cadrays_amd/variants/NAME.so (git-ignored; they travel to the GPU box).  Run with CRH_LIB_PATH=... python bench.py
# The Makefile's variant rule does the work (the product's own objects and flags); at most 6 builds run at a time.
set -e
cd "$(dirname "$0")/../cadrays_amd/csrc"
make -s -j6 all      # the objects every variant shares, before the variants are built side by side
while [ $# -ge 2 ]; do
  NAME=$1; FL=$2; shift 2
  rm -f ../variants/$NAME.so      # same name, other flags: build again
  ( make -s ../variants/$NAME.so VARIANT_DEFS="$FL" 2>/dev/null && echo "built $NAME [$FL]" || echo "FAILED $NAME [$FL]" ) &
  while [ $(jobs -r | wc -l) -ge 6 ]; do sleep 0.5; done
done
wait
