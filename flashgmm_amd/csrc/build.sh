#!/usr/bin/env bash
# Build libflashgmm_amd.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
#   -ffp-contract=off                         : the only fused ops are the explicit FMAs of fgmm_math.h
#   -fhip-fp32-correctly-rounded-divide-sqrt  : IEEE '/' and sqrt on the device (bit-exact CDFs)
#   -march=x86-64-v3                          : host rANS code may use AVX2/BMI2, stays portable across hosts
#   -Xarch_device -fno-slp-vectorize          : packed fp32 ops (v_pk_fma_f32 ...) issue at half rate on gfx950 and cost
#                                               pairing moves: measured 1-6 % (symtab) / 12 % (cdftab count) slower with them
# Sources: the kernels (*.hip; fgmm_encframe.h is the frame fgmm_kernels.hip, fgmm_rate.hip, fgmm_rdoq.hip and fgmm_rdcurve.hip share,
# fgmm_headframe.h the one fgmm_head.hip and fgmm_head16.hip share: placement, rank prologue, epilogues, launch geometry and ladder,
# fgmm_mfma32.h the binary32 matrix-core tile of fgmm_head.hip and fgmm_ckbd_ctx.hip - pitches, fragments, staging, the fenced K loop -
# whose fragments fgmm_ckbd_ctx_grad.hip reads too, fgmm_ckbd_geom.h the checkerboard's taps and positions and the rule for a block's row tiles,
# fgmm_decframe.h the one of the decode-side kernels of fgmm_tab.hip: a latent's parameters, window, pair of edges, trimming, ladder), the device layer over HIP (fgmm_device_hip.cpp), and the host side, which sees the device only
# through fgmm_device.h (fgmm_capi / fgmm_encode / fgmm_decode / fgmm_decode_gpu / fgmm_rans: plain C++, also built without a GPU
# toolchain against tests/fake/fake_device.cpp by scripts/tsan_host.sh); fgmm_rate_host.cpp (the coded size of a table, integer only) and
# fgmm_estimate.cpp / fgmm_rdoq.cpp / fgmm_rdcurve.cpp (the size estimate's, the RDOQ call's and the curve and budget calls' orchestration
# over fgmm_rate.hip / fgmm_rdoq.hip / fgmm_rdcurve.hip, all on the one frame fgmm_estimate.cpp holds - validation, the entry points' shell,
# the census front half: not part of the fake-device build); fgmm_like.cpp over fgmm_like.hip (the entropy model's forward(): likelihood, rate and
# gradients on the encode frame, in the same entry-point shell, without the census: not part of the fake-device build either);
# fgmm_centroid.cpp over fgmm_centroid.hip (centroid reconstruction of decoded latents, section 3i of the header: like_kernel's forward with one
# more sum, in the same shell: not part of the fake-device build either); fgmm_eb.cpp over fgmm_eb.hip (the entropy bottleneck's forward(),
# section 3j: the factorized density of the hyper-latent, its rate and gradients, and its update(), section 3k: the quantile search and the
# masses of the coding tables: not part of the fake-device build either); fgmm_ckbd_ctx.cpp over fgmm_ckbd_ctx.hip
# (the checkerboard context convolution on the matrix cores, section 5b: a weights handle and a stream-ordered apply, on fgmm_headframe.h's
# placement and bias helpers: not part of the fake-device build either; fgmm_ckbd_ctx_grad.hip: its weight and bias gradients, section 5c,
# behind the same fgmm_ckbd_ctx.cpp).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${OUT:-../libflashgmm_amd.so}
COMMON="-O3 -fPIC -std=c++17 -Wall -Wextra -Wno-unused-parameter -ffp-contract=off -fno-fast-math"
$HIPCC $COMMON --offload-arch=gfx950 -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-rdc -Xarch_device -fno-slp-vectorize \
    -march=x86-64-v3 -shared -o $OUT fgmm_kernels.hip fgmm_tab.hip fgmm_head.hip fgmm_head16.hip fgmm_rate.hip fgmm_rdoq.hip fgmm_rdcurve.hip fgmm_like.hip fgmm_centroid.hip fgmm_eb.hip fgmm_ckbd_ctx.hip fgmm_ckbd_ctx_grad.hip fgmm_device_hip.cpp fgmm_rans.cpp fgmm_rate_host.cpp fgmm_capi.cpp \
    fgmm_encode.cpp fgmm_decode.cpp fgmm_decode_gpu.cpp fgmm_estimate.cpp fgmm_rdoq.cpp fgmm_rdcurve.cpp fgmm_like.cpp fgmm_centroid.cpp fgmm_eb.cpp fgmm_ckbd_ctx.cpp -lpthread "$@"
echo "built $(realpath $OUT)"
# The compiled Python boundary over the C ABI (fgmm_pybind.cpp -> flashgmm_amd/_native.*.so): plain C++ against the Python and pybind11
# headers, linked to the library above through an $ORIGIN rpath.  Skipped (the ctypes binding, flashgmm_amd/_lib.py, binds the same
# ABI) when OUT names another library (A/B builds) or the headers are not there.
if [ "$OUT" = "../libflashgmm_amd.so" ] && PYINC=$(python3-config --includes 2>/dev/null) && PB=$(python3 -c 'import pybind11; print(pybind11.get_include())' 2>/dev/null); then
  EXT=$(python3-config --extension-suffix)
  ${CXX:-g++} -O2 -fPIC -shared -std=c++17 -Wall -fvisibility=hidden $PYINC -I"$PB" fgmm_pybind.cpp -o ../_native$EXT -L.. -lflashgmm_amd -Wl,-rpath,'$ORIGIN'
  echo "built $(realpath ../_native$EXT)"
else
  echo "(flashgmm_amd/_native not built: pybind11 / Python headers missing or OUT set - the ctypes binding is used)"
fi
