#!/bin/bash
# Build libffcv_hip.so of a git revision into build/ab/<name>.so (A/B baseline),
# from the files that revision had: its sources and its own build recipe
# (SOURCES and FLAGS of its ffcv_amd/_build.py, loaded by path).
#   tools/build_rev.sh <name> <rev> [extra hipcc flags]
set -e
NAME=$1; REV=$2; shift 2
T=$(mktemp -d)
trap 'rm -rf $T' EXIT
git archive $REV ffcv_amd/csrc ffcv_amd/_build.py include | tar -x -C $T
mkdir -p build/ab
python3 - $T/ffcv_amd/_build.py $(pwd)/build/ab/$NAME.so "$@" <<'PY'
import importlib.util
import os
import subprocess
import sys

path, out, extra = sys.argv[1], sys.argv[2], sys.argv[3:]
spec = importlib.util.spec_from_file_location('_build_of_rev', path)
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)
hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
subprocess.check_call([hipcc] + b.FLAGS + extra + ['-o', out] + b.SOURCES, cwd=b.CSRC)
print(out)
PY
