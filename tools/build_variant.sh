#!/bin/bash
# Build an A/B variant of libffcv_hip.so with extra defines into build/ab/:
# the product's own recipe (ffcv_amd/_build.py) with another output.
#   tools/build_variant.sh <name> -DJW=2 ...   (then bench.py --lib build/ab/<name>.so)
set -e
NAME=$1; shift
python3 -m ffcv_amd._build --out build/ab/$NAME.so -- "$@"
