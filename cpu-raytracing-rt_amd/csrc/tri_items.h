// tri_items.h — one triangle of the scene as build_scene computes it: the Triangle
// (triangle.rs), the vertices it was built from and its box.  The functions are RT_HD so
// that scene_build.cpp's item loop and tri_items.hip's ti_items run one definition,
// operation for operation: plain /, sqrt and no fused multiply-add (-ffp-contract=off),
// so the device's results are the host's bits (NaN payloads aside, DESIGN.md §2
// "Device items").
#pragma once
#include <type_traits>

#include "rt_math.h"

namespace rt {

struct Triangle {            // triangle.rs:5-17
    V3 a, ba, ca, ng;
    double inv_area;
    V3 na, nb, nc;
};

// One triangle of the scene in list order.  bvh_emit.hip reads the records by 16-byte
// loads, hence the alignment.
struct alignas(16) TriItem { Triangle t; V3 b, c; uint32_t mat; int32_t gid; Box3 box; };  // b, c: the vertices t was built from
static_assert(sizeof(TriItem) == 288 && std::is_trivially_copyable<TriItem>::value && std::is_standard_layout<TriItem>::value,
              "TriItem is a POD of 36 eight-byte words (bvh_emit.hip and tri_items.hip index them)");

RT_HD Triangle triangle_props(V3 a, V3 b, V3 c) {                        // triangle.rs:41-47
    Triangle t;
    t.a = a;
    t.ba = b - a;
    t.ca = c - a;
    V3 sized = cross(t.ba, t.ca);
    double area = sqrt(dot(sized, sized)) / 2.0;
    t.ng = normalize(sized);
    t.inv_area = 1.0 / area;
    return t;
}
RT_HD Triangle triangle_smooth(V3 a, V3 b, V3 c, V3 na, V3 nb, V3 nc) {  // triangle.rs:20-23
    Triangle t = triangle_props(a, b, c);
    t.na = na; t.nb = nb; t.nc = nc;
    return t;
}
RT_HD Triangle triangle_geometric(V3 a, V3 b, V3 c) {                    // triangle.rs:25-28
    Triangle t = triangle_props(a, b, c);
    t.na = t.ng; t.nb = t.ng; t.nc = t.ng;
    return t;
}

// RT_TRI_GLTF: new_with_smooth_normal + instantiate (gltf/scene_builder.rs:42-55).
// Fills t, b, c and box; mat and gid are the caller's.
RT_HD void tri_item_gltf(V3 a, V3 b, V3 c, V3 na, V3 nb, V3 nc, TriItem& it) {
    it.t = triangle_smooth(a, b, c, na, nb, nc);
    it.b = b;
    it.c = c;
    Box3 bx = box_empty();
    box_extend(bx, it.t.a);
    box_extend(bx, it.t.a + it.t.ba);
    box_extend(bx, it.t.a + it.t.ca);
    it.box = bx;
}
// RT_TRI_CUSTOM: new_with_geometry_normals (scene_parser.rs:71-73) + TrianglePrimitive::new
// (scene.rs:139-165).  A description without positions / rotations passes 0 / identity,
// and the arithmetic still runs (rotate by identity is no no-op on -0.0).
RT_HD void tri_item_custom(V3 va, V3 vb, V3 vc, V3 pos, Quat rot, TriItem& it) {
    Triangle m = triangle_geometric(va, vb, vc);
    V3 a = rotate(rot, m.a) + pos;
    V3 b = rotate(rot, m.ba + m.a) + pos;
    V3 c = rotate(rot, m.ca + m.a) + pos;
    it.t = triangle_smooth(a, b, c, rotate(rot, m.na), rotate(rot, m.nb), rotate(rot, m.nc));
    it.b = b;
    it.c = c;
    Box3 bb = box_empty();
    box_extend(bb, a); box_extend(bb, b); box_extend(bb, c);
    it.box = bb;
}

}  // namespace rt
