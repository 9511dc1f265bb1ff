// mc_vertex.h -- the one vertex formula of the dense (mesh.hip) and the sparse
// (mesh_sparse.hip) marching cubes, so that the two meshes carry the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfr {

// vertex of grid edge (axis d) from point (i, j, k): the low end plus
// t = (level - v_a) / (v_b - v_a) along d, in fp32 with one rounding per op
__device__ __forceinline__ void put_vertex(float *verts, uint32_t id, uint32_t i, uint32_t j,
                                           uint32_t k, int d, float va, float vb, float level) {
    const float t = __fdiv_rn(__fsub_rn(level, va), __fsub_rn(vb, va));
    float x = (float)i, y = (float)j, z = (float)k;
    if (d == 0) x = __fadd_rn(x, t);
    else if (d == 1) y = __fadd_rn(y, t);
    else z = __fadd_rn(z, t);
    verts[3ull * id + 0] = x;
    verts[3ull * id + 1] = y;
    verts[3ull * id + 2] = z;
}

}  // namespace sdfr
