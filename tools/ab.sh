#!/bin/bash
# A/B kernel variants: tools/ab.sh <frames> <reps> v1 v2 ...   (libraries var/libfxcorr_<v>.so: build/ is not shipped to the GPU box)
# Three alternating rounds; the same library under two names (a copy) gives the A/A spread of the call.  A run that fails or
# outlasts its time limit ends the whole comparison: nothing more is started on the GPU after it.
frames=$1; reps=$2; shift 2
for round in 1 2 3; do
for v in "$@"; do
  FXCORR_LIB=$PWD/var/libfxcorr_$v.so timeout -k 10 300 python tools/kbench.py --frames $frames --reps $reps --tag $v || exit $?
done
done
