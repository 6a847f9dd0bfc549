// bvh_device.h — what bvh_build.hip and bvh_emit.hip share: the builder's tree as it
// stays in device memory, and the per-call scratch arena that owns it.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "scene_build.h"

namespace rt {

struct OutNode { double box[6]; int64_t left, right; uint64_t start, end; };  // HostNode's bytes
static_assert(sizeof(OutNode) == sizeof(HostNode) && sizeof(OutNode) == 80, "OutNode mirrors HostNode");

struct Arena {  // per-call scratch: everything is freed before the call returns
    std::vector<void*> ptrs;
    bool oom = false;
    hipError_t err = hipSuccess;
    ~Arena() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T>
    T* get(size_t count) {
        void* p = nullptr;
        if (oom || err != hipSuccess) return nullptr;
        const hipError_t e = hipMalloc(&p, (count ? count : 1) * sizeof(T));
        if (e == hipErrorOutOfMemory) { oom = true; (void)hipGetLastError(); return nullptr; }
        if (e != hipSuccess) { err = e; return nullptr; }
        ptrs.push_back(p);
        return (T*)p;
    }
    void release(void* p) {
        for (void*& q : ptrs) if (q == p && p) { (void)hipFree(p); q = nullptr; }
    }
    // everything taken since `mark` (ptrs.size() then) except the two kept
    void release_since(size_t mark, const void* keep0, const void* keep1) {
        for (size_t i = mark; i < ptrs.size(); ++i)
            if (ptrs[i] && ptrs[i] != keep0 && ptrs[i] != keep1) { (void)hipFree(ptrs[i]); ptrs[i] = nullptr; }
    }
    bool ok() const { return !oom && err == hipSuccess; }
};

// The tree of build_bvh over n boxes, left on the device: nodes in pre-order (inner nodes
// with start = end = 0) and the leaf primitive order.  Both belong to the arena.
struct DevTree {
    OutNode* nodes = nullptr;
    uint32_t* order = nullptr;
    uint32_t n_nodes = 0, depth = 0;
};
// bvh_build.hip: build_bvh_device without the copies.  d_boxes: n boxes (six doubles each,
// list order) in device memory, 1 <= n <= 2^30.  Returns as build_bvh_device does; on
// kDeviceBuildDone the builder's own scratch is already released and the stream is idle.
int build_bvh_device_tree(Arena& m, const double* d_boxes, uint32_t n, uint32_t max_levels, DevTree& out,
                          std::string& err);

// bvh_emit.hip: emit_tri_bvh_device behind its upload.  d_items (n triangles in list order)
// and d_boxes (their boxes, six doubles each) are device memory of the caller's arena;
// d_boxes is released once the tree stands, and whatever the call itself took from the
// arena is released before it returns, so a caller may emit several BVHs in turn.  Returns
// as emit_tri_bvh_device does (n == 0: kDeviceBuildFallback).
int emit_tri_bvh_device_core(Arena& m, const TriItem* d_items, double* d_boxes, uint32_t n, bool compact,
                             uint32_t max_levels, HostBvhArrays& out, std::string& err);

// What the item kernels (tri_items.hip ti_items, gltf_items.hip gf_items and gf_scan) leave
// for the host: the triangles queued for the NaN fix-up, the light triangles, and
// gf_scan's findings (kScanNonFinite | kScanIndexRange; 0 from ti_items).
struct ItemsHeader { uint32_t n_nan, n_light, scan; };
enum : uint32_t { kScanNonFinite = 1u, kScanIndexRange = 2u };
// tri_items.hip: clears the header (a kernel on `st`; launch before the item kernel).
void items_header_clear(ItemsHeader* d_hdr, hipStream_t st);
// tri_items.hip: the tail that both item front ends share, called with the item kernel
// launched on stream 0 and all of it in the caller's arena: d_items / d_boxes the n items,
// d_mat the material of each, d_light a byte per material (is_light), d_queue the fix-up
// queue (kFixCap words), d_hdr the header.  Counts and compacts the light triangles,
// releases `inputs` once the item kernel is through, patches in the queued items as
// item_of(ctx, j, item) computes them on the host, and emits both triangle BVHs.  Returns
// and fills res as a TriBvhItems does; a non-zero header.scan is kDeviceBuildFallback.
int finish_device_items(Arena& m, uint32_t n, TriItem* d_items, double* d_boxes, uint32_t* d_mat, uint8_t* d_light,
                        uint32_t* d_queue, ItemsHeader* d_hdr, void* const* inputs, uint32_t n_inputs,
                        void (*item_of)(const void* ctx, uint32_t j, TriItem& it), const void* ctx, uint32_t max_levels,
                        HostBvhArrays& tris, HostBvhArrays& ltris, TriItemsOutcome& res, std::string& err);

}  // namespace rt

// -DRT_EMIT_TIMES (a variant build): the wall time of each phase of an emission on stderr
#ifdef RT_EMIT_TIMES
#define RT_EMIT_MARK_START() auto mark_ = std::chrono::steady_clock::now()
#define RT_EMIT_MARK(name)                                                                         \
    do {                                                                                           \
        (void)hipDeviceSynchronize();                                                              \
        const auto now_ = std::chrono::steady_clock::now();                                        \
        fprintf(stderr, "  emit %-14s %8.1f ms\n", name, std::chrono::duration<double, std::milli>(now_ - mark_).count()); \
        mark_ = now_;                                                                              \
    } while (0)
#else
#define RT_EMIT_MARK_START() do {} while (0)
#define RT_EMIT_MARK(name) do {} while (0)
#endif
