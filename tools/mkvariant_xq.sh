#!/bin/bash
# mkvariant_xq.sh <name> [-D...]: libwoq_hip.so with the XQ decode GEMV (woq_gemv_xq.hip) compiled under extra switches
# -> tools/lib_xq_<name>.so; select with WOQ_HIP_LIB=<path>. The one switch left is the stage-stamp build read by
# tools/xqs_stamps.py: tools/mkvariant_xq.sh stamps -DWOQ_XQS_STAMPS
set -e
cd "$(dirname "$0")/../intel_extension_for_transformers_amd/csrc"
name=$1; shift
make -j8 >/dev/null
FL="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -mllvm -amdgpu-kernarg-preload-count=14 -fvisibility=hidden -Wno-unused-value"
/opt/rocm/bin/hipcc $FL "$@" -c woq_gemv_xq.hip -o _build/varxq_$name.o
objs=$(ls _build/woq_*.o | grep -v "woq_gemv_xq.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs _build/varxq_$name.o -o ../../tools/lib_xq_$name.so
echo built tools/lib_xq_$name.so
