// canting_basis.hpp - the orthonormal facet basis of the canting rotation (artist/geometry/transforms.py:320-340), shared by
// nurbs_kernels.hip (the fused evaluation) and canting_kernels.hip (the rotation on its own, with its gradients): one copy, so
// that both translation units rotate with the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "nurbs_basis.hpp"   // norm3

namespace art {

// transforms.py:320-340.  B[0..2] = e, B[3..5] = n_ortho, B[6..8] = u.
__device__ __forceinline__ void canting_basis(const float* cant, float* B)
{
    float ex = cant[0], ey = cant[1], ez = cant[2];
    const float nx = cant[4], ny = cant[5], nz = cant[6];
    const float ne = fmaxf(norm3(ex, ey, ez), 1e-12f);
    ex = ex / ne; ey = ey / ne; ez = ez / ne;
    float ux = ey * nz - ez * ny, uy = ez * nx - ex * nz, uz = ex * ny - ey * nx;
    const float nu_ = fmaxf(norm3(ux, uy, uz), 1e-8f);
    ux = ux / nu_; uy = uy / nu_; uz = uz / nu_;
    float ox = uy * ez - uz * ey, oy = uz * ex - ux * ez, oz = ux * ey - uy * ex;
    const float no = fmaxf(norm3(ox, oy, oz), 1e-8f);
    ox = ox / no; oy = oy / no; oz = oz / no;
    B[0] = ex; B[1] = ey; B[2] = ez; B[3] = ox; B[4] = oy; B[5] = oz; B[6] = ux; B[7] = uy; B[8] = uz;
}

}  // namespace art
