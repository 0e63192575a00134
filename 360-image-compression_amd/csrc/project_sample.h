// project_sample.h -- the per-element arithmetic of ProjectsOp's forward (extension/projects_cuda.cu:181-232), shared by k_projects_forward
// (project_kernels.hip) and the fused viewport metrics (viewport_quality_kernels.hip) so that both sample the very same numbers: one
// sampling coordinate f = (x, y) in ERP pixels, one image plane [hs][ws] -> one sample.  The unit is built without contraction, so the
// products and sums below round one by one, left to right.  lic360_project_scatter is its adjoint, for the backward of the fused viewport metrics.
#pragma once
#include <hip/hip_runtime.h>

template <bool NEAREST>
__device__ __forceinline__ float lic360_project_sample(const float *__restrict__ img, float2 f, int hs, int ws) {
    if constexpr (NEAREST) {
        const int tw = (int)floor((double)f.x + 0.5) % ws;
        int th = (int)floor((double)f.y + 0.5);
        th = th >= hs ? hs - 1 : th;
        return img[th * ws + tw];
    } else {
        const int tw = (int)floorf(f.x), th = (int)floorf(f.y);
        const int pw = (tw + 1) % ws, ph = th + 1 >= hs ? hs - 1 : th + 1;
        const float tx = f.x - tw, ty = f.y - th, ntx = (float)(1. - tx), nty = (float)(1. - ty);
        return img[th * ws + tw] * ntx * nty + img[th * ws + pw] * tx * nty + img[ph * ws + tw] * ntx * ty + img[ph * ws + pw] * tx * ty;
    }
}

// The adjoint of lic360_project_sample: the gradient g of one sample is added to the cells of the plane `grad` it was read from, with the indices and
// weights above and the products of k_projects_backward (weight * weight * g, left to right); four float atomic adds, one when NEAREST.
template <bool NEAREST>
__device__ __forceinline__ void lic360_project_scatter(float *grad, float2 f, int hs, int ws, float g) {
    if constexpr (NEAREST) {
        const int tw = (int)floor((double)f.x + 0.5) % ws;
        int th = (int)floor((double)f.y + 0.5);
        th = th >= hs ? hs - 1 : th;
        atomicAdd(grad + th * ws + tw, g);
    } else {
        const int tw = (int)floorf(f.x), th = (int)floorf(f.y);
        const int pw = (tw + 1) % ws, ph = th + 1 >= hs ? hs - 1 : th + 1;
        const float tx = f.x - tw, ty = f.y - th, ntx = (float)(1. - tx), nty = (float)(1. - ty);
        atomicAdd(grad + th * ws + tw, ntx * nty * g);
        atomicAdd(grad + th * ws + pw, tx * nty * g);
        atomicAdd(grad + ph * ws + tw, ntx * ty * g);
        atomicAdd(grad + ph * ws + pw, tx * ty * g);
    }
}
