// gltf_math.h — the flatten arithmetic of a glTF primitive (gltf/scene_builder.rs:269-327)
// and the draw plan it runs over.  The functions are RT_HD so that gltf.cpp's host flatten
// and gltf_items.hip's gf_items run one definition, operation for operation: f32 -> f64,
// plain *, +, / and sqrt in cgmath's order, no fused multiply-add (-ffp-contract=off), so
// the device's vertices and normals are the host's bits (NaN payloads aside, DESIGN.md §2
// "Device meshes").
#pragma once
#include "rt_math.h"

namespace rt {

// Row r of Matrix4 * Vector4(x, y, z, 1.0): m is cgmath's column-major m[c * 4 + r].
RT_HD double gltf_row(const double* m, int r, double x, double y, double z) {
    return ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * 1.0;
}
// read_vertices: the f32 position through the node matrix (rows 0..2)
RT_HD V3 gltf_point(const double* m, float fx, float fy, float fz) {
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    return v3(gltf_row(m, 0, x, y, z), gltf_row(m, 1, x, y, z), gltf_row(m, 2, x, y, z));
}
// read_normals: the f32 normal through the cofactor matrix rs[c * 3 + r], normalised
RT_HD V3 gltf_normal(const double* rs, float fx, float fy, float fz) {
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const V3 n = v3((rs[0] * x + rs[3] * y) + rs[6] * z, (rs[1] * x + rs[4] * y) + rs[7] * z,
                    (rs[2] * x + rs[5] * y) + rs[8] * z);
    return normalize(n);
}

// One converted primitive of a deferred glTF parse, in convert_node order.  Every accessor
// is checked at planning: its last element lies inside its buffer, offsets and strides are
// multiples of the component size, the node matrix's row 3 is (+-0, +-0, +-0, 1).
struct GltfDraw {
    double m[16];                          // node matrix, column-major
    double cof[9];                         // cof() of its upper-left 3x3, [col][row]
    uint64_t pos_off, nrm_off, idx_off;    // bytes from the start of the buffer; in the device's table, of the blob
    uint32_t pos_stride, nrm_stride, idx_stride;
    uint32_t idx_width;                    // 0: not indexed; 2: u16; 4: u32
    uint32_t n_verts, n_idx;               // POSITION's (= NORMAL's) count, the index count
    uint32_t n_tris, first_tri;            // first_tri: the scene's triangles before this draw
    uint32_t mid;                          // the draw's material
    uint32_t pos_buf, nrm_buf, idx_buf;    // which of the parse's buffers
};
static_assert(sizeof(GltfDraw) == 272, "GltfDraw is uploaded as it is");

}  // namespace rt
