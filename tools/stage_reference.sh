#!/bin/bash
# Stage the reference checkout into oracle/_ref/ (git-ignored, never committed): the recipe build() runs too
# (oracle/Makefile `ref`).  The drop-in acceptance tests (-m gpu) run the copy.   usage: stage_reference.sh [<mpyc checkout>]
set -e
cd "$(dirname "$0")/.."
make -C oracle ref ${1:+MPYC_REFERENCE="$1"}
du -sh oracle/_ref
