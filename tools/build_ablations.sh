#!/bin/bash
# Side builds of the engine with extra compiler flags, for experiments: tools/build_ablations.sh NAME -DFLAG...
# (-DGWI_PBATCH_U=..., -DGWI_SCAN_WAVES_PER_EU=..., -DGWI_STAMPS for tools/stamp_phases.py, the short variant tables of
# gwi_engine.hip for a quick build)
# -> gwinferno_amd/_lib_NAME/{libgwi_engine.so,gwi_kernels.hsaco}; run with GWI_ENGINE_LIB=gwinferno_amd/_lib_NAME/libgwi_engine.so
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
out=$R/gwinferno_amd/_lib_$name; mkdir -p $out
F="--offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -mllvm -amdgpu-kernarg-preload-count=16 -I$R/include -I$R/gwinferno_amd/csrc $@"
/opt/rocm/bin/hipcc $F -fPIC -shared -o $out/libgwi_engine.so $R/gwinferno_amd/csrc/gwi_engine.hip $R/gwinferno_amd/csrc/gwi_sampler.cpp -ldl -lpthread 2>/dev/null &
/opt/rocm/bin/hipcc $F --cuda-device-only --no-gpu-bundle-output -o $out/gwi_kernels.hsaco $R/gwinferno_amd/csrc/gwi_engine.hip 2>/dev/null &
wait
ls -la $out
