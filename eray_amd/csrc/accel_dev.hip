// accel_dev.hip — the ray-query hierarchy built on the device (accel_dev.hpp) from the resident
// TriHot records, for gfx950.  The arithmetic is accel_margin.hpp's and accel_layout.hpp's, the
// code tests/cpp/accel_dev_main.cpp runs on the CPU; this file adds the data movement.
//
// Every covered object's faces are numbered g = gbegin + k (k: the index within the object) over
// the covered objects in scene order; gbegin is also the object's first slot, as in the host
// build.  All kernels work on every covered object at once; a workgroup never straddles objects.
//
//   margin_kernel   one face per lane: face_margin_of in FP64 -> unculled flag, (alpha, beta);
//                   centroid bounds, max gamma and the counts reduced per wave (shuffles), per
//                   workgroup (LDS), then one vector atomic each on order-preserving u64 encodings
//   exclusive scan  of the flags (rocprim): S[g] = unculled faces before g
//   key_kernel      unculled face -> slot gbegin + S[g] - S[gbegin] (ascending index), record and
//                   index copied; culled face -> (Morton key, g) at p = g - S[g]
//   radix sort      of (key, g) by the 63 key bits (rocprim, stable: ties stay in index order);
//                   with several objects a second stable pass by object ordinal regroups them
//   level_kernel    one launch per level, deepest first, one node per lane: leaves (make_leaf) and
//                   inner nodes (make_inner) exactly as accel_layout.hpp lays them out
//   object_kernel   the Object records
//
// accel_refit_device keeps a built topology for moved faces: margin_kernel, refit_check_kernel (the
// unculled lists are still exact), the same read-back, refit_level_kernel per level over the
// hierarchy's own index array, object_kernel — no scan, no keys, no sort, no allocation that stays.
// accel_refit_enqueue is that refit with the host taken out (a persistent workspace, the verdict by
// refit_object_kernel, the levels of at most kBlock nodes by refit_top_levels_kernel in one launch):
// kernels on the stream only, so that a graph can hold it.  Both also refit a tree the host builder
// made (eray_scene_build_ray_accel_refittable): the same shape numbered in recursion order, for which
// the level kernels have a second instantiation (…_preorder_kernel) picked by the layout's numbering.
//
// The host reads back 16 B of counters per covered object after key_kernel (it needs the culled
// counts to size the node array and lay out the levels); nothing else crosses the bus.
#include "accel_dev.hpp"

#include <algorithm>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "accel_layout.hpp"

namespace eray {
namespace gpu {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWaves = kBlock / 64;

using DevObj = AccelDevLayout;  // 48 B (accel_layout.hpp; RayAccel keeps the build's for the refit)
static_assert(sizeof(DevObj) == 48, "uploaded as it stands");

struct DevAcc {  // 64 B
    unsigned long long lo[3], hi[3], gamma, pad;
};
// Before a margin pass: lo at all ones, the rest at zero.  (refit_reset_kernel keeps the literal:
// through this function its code comes out different.)
ERAY_HD DevAcc dev_acc_start() { return DevAcc{{~0ull, ~0ull, ~0ull}, {0, 0, 0}, 0, 0}; }

struct DevCount {  // the block the host reads back
    uint32_t culled, unculled, status, pad;
};

// doubles as unsigned integers of the same order
__device__ inline unsigned long long enc(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double dec(unsigned long long e) {
    const unsigned long long b = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    return __longlong_as_double((long long)b);
}

// the covered object of workgroup `block` (workgroup-uniform)
__device__ inline uint32_t object_of_block(const DevObj* objs, uint32_t n, uint32_t block) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (objs[mid].block_begin <= block) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ inline accel::Hot load_hot(const TriHot* p) {
    const float4 a = p->q0, b = p->q1, c = p->q2;  // three 16-B loads
    return accel::Hot{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w}};
}
__device__ inline void store_hot(accel::Hot* p, const accel::Hot& r) {
    float4* q = reinterpret_cast<float4*>(p);
    q[0] = make_float4(r.q[0], r.q[1], r.q[2], r.q[3]);
    q[1] = make_float4(r.q[4], r.q[5], r.q[6], r.q[7]);
    q[2] = make_float4(r.q[8], r.q[9], r.q[10], r.q[11]);
}

__device__ inline double wave_min(double v) {
    for (int m = 32; m; m >>= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int m = 32; m; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

__global__ __launch_bounds__(kBlock) void margin_kernel(const TriHot* __restrict__ tris, const DevObj* __restrict__ objs,
                                                        uint32_t nobj, uint32_t* __restrict__ flags,
                                                        double2* __restrict__ alpha_beta, DevAcc* __restrict__ acc,
                                                        DevCount* __restrict__ cnt) {
    __shared__ double s_red[kWaves][7];
    __shared__ uint32_t s_cnt[kWaves][2];
    const uint32_t o = object_of_block(objs, nobj, blockIdx.x);
    const DevObj ob = objs[o];
    const uint32_t k = (blockIdx.x - ob.block_begin) * kBlock + threadIdx.x;
    const bool active = k < ob.faces;
    double v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
    bool culled = false;
    if (active) {
        const accel::Hot r = load_hot(tris + ob.hot_begin + k);
        const accel::FaceMargin m = accel::face_margin_of(r);
        culled = m.culled;
        const uint32_t g = ob.gbegin + k;
        flags[g] = culled ? 0u : 1u;
        alpha_beta[g] = make_double2(m.alpha, m.beta);
        if (culled) {
            double c[3];
            accel::centroid_of(r, c);
            for (int j = 0; j < 3; ++j) v[j] = v[3 + j] = c[j];
            v[6] = m.gamma;
        }
    }
    const uint32_t nc = (uint32_t)__popcll(__ballot(active && culled)), nu = (uint32_t)__popcll(__ballot(active && !culled));
    for (int j = 0; j < 3; ++j) v[j] = wave_min(v[j]);
    for (int j = 3; j < 7; ++j) v[j] = wave_max(v[j]);
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0) {
        for (int j = 0; j < 7; ++j) s_red[wave][j] = v[j];
        s_cnt[wave][0] = nc;
        s_cnt[wave][1] = nu;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int j = (int)threadIdx.x;
        double x = s_red[0][j];
        for (uint32_t w = 1; w < kWaves; ++w) x = j < 3 ? fmin(x, s_red[w][j]) : fmax(x, s_red[w][j]);
        uint32_t any = 0;
        for (uint32_t w = 0; w < kWaves; ++w) any += s_cnt[w][0];
        if (any) {  // (no culled face: nothing to record)
            if (j < 3) atomicMin(&acc[o].lo[j], enc(x));
            else if (j < 6) atomicMax(&acc[o].hi[j - 3], enc(x));
            else atomicMax(&acc[o].gamma, enc(x));
        }
    } else if (threadIdx.x < 9) {
        const uint32_t j = threadIdx.x - 7;
        uint32_t x = 0;
        for (uint32_t w = 0; w < kWaves; ++w) x += s_cnt[w][j];
        if (x) atomicAdd(j ? &cnt[o].unculled : &cnt[o].culled, x);
    }
}

__global__ __launch_bounds__(kBlock) void key_kernel(const TriHot* __restrict__ tris, const DevObj* __restrict__ objs,
                                                     uint32_t nobj, const uint32_t* __restrict__ flags,
                                                     const uint32_t* __restrict__ scan, const DevAcc* __restrict__ acc,
                                                     unsigned long long* __restrict__ keys,
                                                     uint32_t* __restrict__ ids, accel::Hot* __restrict__ hot,
                                                     uint32_t* __restrict__ index) {
    const uint32_t o = object_of_block(objs, nobj, blockIdx.x);
    const DevObj ob = objs[o];
    const uint32_t k = (blockIdx.x - ob.block_begin) * kBlock + threadIdx.x;
    if (k >= ob.faces) return;
    const uint32_t g = ob.gbegin + k;
    const uint32_t before = scan[g];
    const accel::Hot r = load_hot(tris + ob.hot_begin + k);
    const bool unculled = flags[g] != 0u;
    if (unculled) {
        const uint32_t slot = ob.gbegin + (before - scan[ob.gbegin]);
        store_hot(hot + slot, r);
        index[slot] = k;
        return;
    }
    const DevAcc a = acc[o];
    const double lo[3] = {dec(a.lo[0]), dec(a.lo[1]), dec(a.lo[2])}, hi[3] = {dec(a.hi[0]), dec(a.hi[1]), dec(a.hi[2])};
    double c[3];
    accel::centroid_of(r, c);
    const uint32_t p = g - before;
    keys[p] = accel::morton_key(c, lo, hi);
    ids[p] = g;
}

// the covered object of face g
__global__ __launch_bounds__(kBlock) void ordinal_kernel(const DevObj* __restrict__ objs, uint32_t nobj,
                                                         const uint32_t* __restrict__ ids, uint32_t n,
                                                         uint32_t* __restrict__ ord) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t g = ids[p];
    uint32_t lo = 0, hi = nobj;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (objs[mid].gbegin <= g) lo = mid; else hi = mid;
    }
    ord[p] = lo;
}

// Level `level` (0: the roots) of every covered object's tree, objects obj0 + blockIdx.y: a
// complete level's nodes, or (level == full + 1) the pairs of leaves under the nodes of level
// `full` that split once more — one parent per lane.  Deeper levels are written.
__global__ __launch_bounds__(kBlock) void level_kernel(uint32_t level, uint32_t obj0, const TriHot* __restrict__ tris,
                                                       const DevObj* __restrict__ objs, const uint32_t* __restrict__ ids,
                                                       const double* __restrict__ alpha_beta, accel::Node* nodes,
                                                       accel::NodeBounds* bounds, accel::Hot* __restrict__ hot,
                                                       uint32_t* __restrict__ index) {
    const DevObj ob = objs[obj0 + blockIdx.y];
    const accel::TreeLayout t{ob.C, ob.full, ob.extra, 0u, 0u};
    accel::level_node(t, level, blockIdx.x * kBlock + threadIdx.x, ids + ob.cbase, ob.gbegin,
                      reinterpret_cast<const accel::Hot*>(tris) + ob.hot_begin, alpha_beta + 2 * (size_t)ob.gbegin, ob.node_base,
                      ob.gbegin + ob.U, nodes, bounds, hot, index);
}

// The refit's check of the unculled lists (same grid as margin_kernel; lane k takes the object's
// k-th unculled slot): the face a slot lists must still be flagged unculled — with the per-object
// unculled count unchanged (the host compares it) the list is then exactly the unculled set again.
// The slot's record copy is refreshed; a slot that fails posts the object's status word.
__global__ __launch_bounds__(kBlock) void refit_check_kernel(const TriHot* __restrict__ tris, const DevObj* __restrict__ objs,
                                                             uint32_t nobj, const uint32_t* __restrict__ flags,
                                                             const uint32_t* __restrict__ index, accel::Hot* __restrict__ hot,
                                                             DevCount* __restrict__ cnt) {
    const uint32_t o = object_of_block(objs, nobj, blockIdx.x);
    const DevObj ob = objs[o];
    const uint32_t k = (blockIdx.x - ob.block_begin) * kBlock + threadIdx.x;
    if (k >= ob.U) return;  // (U <= faces: the slot is the object's)
    const uint32_t slot = ob.gbegin + k, f = index[slot];
    if (f < ob.faces && flags[ob.gbegin + f] != 0u)
        store_hot(hot + slot, load_hot(tris + ob.hot_begin + f));
    else
        atomicOr(&cnt[o].status, 1u);
}

// level_kernel for the refit: the sorted order of an object is the hierarchy's own index array from
// its first culled slot (a leaf's slots hold its range of the order, ascending; make_leaf re-sorts
// them), bias 0.  `index` is read and written — each lane reads its leaves' ranges before it
// writes them, and no two lanes share a range — so neither pointer is __restrict__.
// Numbering: accel_layout.hpp's LevelOrder for a device build, PreOrder for a refittable host build
// (its leaves lie in range order, so its index array is the sorted order just the same).
template <class Numbering>
__device__ __forceinline__ void refit_level(uint32_t level, uint32_t obj0, const TriHot* __restrict__ tris,
                                            const DevObj* __restrict__ objs, const double* __restrict__ alpha_beta,
                                            accel::Node* nodes, accel::NodeBounds* bounds, accel::Hot* __restrict__ hot,
                                            uint32_t* index) {
    const DevObj ob = objs[obj0 + blockIdx.y];
    const accel::TreeLayout t{ob.C, ob.full, ob.extra, 0u, 0u};
    accel::level_node<Numbering>(t, level, blockIdx.x * kBlock + threadIdx.x, index + ob.gbegin + ob.U, 0u,
                                 reinterpret_cast<const accel::Hot*>(tris) + ob.hot_begin, alpha_beta + 2 * (size_t)ob.gbegin,
                                 ob.node_base, ob.gbegin + ob.U, nodes, bounds, hot, index);
}

__global__ __launch_bounds__(kBlock) void refit_level_kernel(uint32_t level, uint32_t obj0, const TriHot* __restrict__ tris,
                                                             const DevObj* __restrict__ objs,
                                                             const double* __restrict__ alpha_beta, accel::Node* nodes,
                                                             accel::NodeBounds* bounds, accel::Hot* __restrict__ hot,
                                                             uint32_t* index) {
    refit_level<accel::LevelOrder>(level, obj0, tris, objs, alpha_beta, nodes, bounds, hot, index);
}

// The same for trees numbered in recursion order: a level's nodes are not contiguous, so its 48-B
// node and 64-B bounds stores scatter over the tree's node range.
__global__ __launch_bounds__(kBlock) void refit_level_preorder_kernel(uint32_t level, uint32_t obj0,
                                                                      const TriHot* __restrict__ tris,
                                                                      const DevObj* __restrict__ objs,
                                                                      const double* __restrict__ alpha_beta, accel::Node* nodes,
                                                                      accel::NodeBounds* bounds, accel::Hot* __restrict__ hot,
                                                                      uint32_t* index) {
    refit_level<accel::PreOrder>(level, obj0, tris, objs, alpha_beta, nodes, bounds, hot, index);
}

__global__ __launch_bounds__(kBlock) void object_kernel(const DevObj* __restrict__ objs, uint32_t nobj,
                                                        const DevAcc* __restrict__ acc, accel::Object* __restrict__ out) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= nobj) return;
    const DevObj ob = objs[o];
    accel::Object r{};
    r.has = 1;
    r.root = ob.C ? ob.node_base : accel::kNoNode;
    r.ubegin = ob.gbegin;
    r.ucount = ob.U;
    r.gamma = accel::up(ob.C ? dec(acc[o].gamma) : 0.0);
    out[ob.index] = r;
}

// ---- the refit on the stream (accel_refit_enqueue): nothing below is read back by the host ----

// The accumulators' and counters' start values, per covered object (DevAcc: lo all ones, the rest 0).
__global__ __launch_bounds__(kBlock) void refit_reset_kernel(DevAcc* __restrict__ acc, DevCount* __restrict__ cnt, uint32_t nobj) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= nobj) return;
    acc[o] = DevAcc{{~0ull, ~0ull, ~0ull}, {0, 0, 0}, 0, 0};  // (dev_acc_start's value)
    cnt[o] = DevCount{0, 0, 0, 0};
}

// refit_level_kernel's levels below first_deep in one launch: one workgroup per covered object
// (obj0 + blockIdx.x), lane j the level's node j, deepest first.  An inner node reads the nodes and
// bounds its children's lanes stored one level earlier, through global memory.  s_barrier waits for
// no counter, and for a workgroup-scope fence the compiler emits no vector-memory wait here, so
// every wave drains its own stores (s_waitcnt vmcnt(0)) before it joins the barrier; the readers
// are waves of the same workgroup — the same CU, whose L1 the stores went through — so no
// agent-scope acquire is needed, and nodes / bounds / index carry no __restrict__, so the compiler
// neither moves nor keeps a load across the fence in __syncthreads().  The bytes are those of the
// per-level passes: the same level_node per (level, lane), each level complete before the next.
// Under either numbering: which ids the children have changes where a lane reads, not who wrote it
// (a lane of this workgroup, one level earlier) nor through what (global memory).
template <class Numbering>
__device__ __forceinline__ void refit_top_levels(uint32_t first_deep, uint32_t obj0, const TriHot* __restrict__ tris,
                                                 const DevObj* __restrict__ objs, const double* __restrict__ alpha_beta,
                                                 accel::Node* nodes, accel::NodeBounds* bounds, accel::Hot* __restrict__ hot,
                                                 uint32_t* index) {
    static_assert(kBlock == accel::kTopBlock, "a level of at most kTopBlock nodes per workgroup");
    const DevObj ob = objs[obj0 + blockIdx.x];
    const accel::TreeLayout t{ob.C, ob.full, ob.extra, 0u, 0u};
    for (uint32_t level = first_deep; level-- > 0;) {  // (workgroup-uniform: every lane meets every barrier)
        accel::level_node<Numbering>(t, level, threadIdx.x, index + ob.gbegin + ob.U, 0u,
                                     reinterpret_cast<const accel::Hot*>(tris) + ob.hot_begin, alpha_beta + 2 * (size_t)ob.gbegin,
                                     ob.node_base, ob.gbegin + ob.U, nodes, bounds, hot, index);
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void refit_top_levels_kernel(uint32_t first_deep, uint32_t obj0, const TriHot* __restrict__ tris,
                                                                  const DevObj* __restrict__ objs,
                                                                  const double* __restrict__ alpha_beta, accel::Node* nodes,
                                                                  accel::NodeBounds* bounds, accel::Hot* __restrict__ hot,
                                                                  uint32_t* index) {
    refit_top_levels<accel::LevelOrder>(first_deep, obj0, tris, objs, alpha_beta, nodes, bounds, hot, index);
}

__global__ __launch_bounds__(kBlock) void refit_top_levels_preorder_kernel(uint32_t first_deep, uint32_t obj0,
                                                                           const TriHot* __restrict__ tris,
                                                                           const DevObj* __restrict__ objs,
                                                                           const double* __restrict__ alpha_beta,
                                                                           accel::Node* nodes, accel::NodeBounds* bounds,
                                                                           accel::Hot* __restrict__ hot, uint32_t* index) {
    refit_top_levels<accel::PreOrder>(first_deep, obj0, tris, objs, alpha_beta, nodes, bounds, hot, index);
}

// The verdict the synchronous refit takes on the host, taken here: per covered object the counters
// against the layout (accel::refit_keeps), the Object record written accordingly (object_kernel's
// on a pass, has = 0 otherwise), the verdict stored; one lane counts the refit.
__global__ __launch_bounds__(kBlock) void refit_object_kernel(const DevObj* __restrict__ objs, uint32_t nobj,
                                                              const DevAcc* __restrict__ acc, const DevCount* __restrict__ cnt,
                                                              accel::Object* __restrict__ out, uint32_t* __restrict__ verdict,
                                                              uint32_t* refits) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o == 0) atomicAdd(refits, 1u);
    if (o >= nobj) return;
    const DevObj ob = objs[o];
    const DevCount c = cnt[o];
    const bool keeps = accel::refit_keeps(c.culled, c.unculled, c.status, ob.C, ob.U);
    out[ob.index] = accel::refit_object(keeps, ob.C, ob.U, ob.node_base, ob.gbegin, keeps && ob.C ? dec(acc[o].gamma) : 0.0);
    verdict[o] = keeps ? 1u : 0u;
}

// one allocation carved into aligned pieces
struct Arena {
    DeviceBuf<unsigned char> mem;
    size_t need = 0;
    size_t reserve(size_t bytes) {
        const size_t at = need;
        need += (bytes + 255) / 256 * 256;
        return at;
    }
    hipError_t alloc() { return mem.alloc(std::max<size_t>(need, 256)); }
    template <typename T>
    T* at(size_t offset) const {
        return reinterpret_cast<T*>((unsigned char*)mem + offset);
    }
};

#define TRY(expr)                       \
    do {                                \
        const hipError_t e_ = (expr);   \
        if (e_ != hipSuccess) return e_; \
    } while (0)

// The numbering of a layout's trees (one build call made them all): recursion order or level order.
bool preorder(const std::vector<DevObj>& objs) { return !objs.empty() && objs.front().numbering == 1u; }

// Levels [first, depth) of every covered object's tree by `pass` (a level kernel: level, obj0, then
// args), deepest first, the objects in chunks of at most 65,535 per grid.y.
template <typename... Params, typename... Args>
hipError_t launch_levels(void (*pass)(uint32_t, uint32_t, Params...), uint32_t first, uint32_t depth, uint32_t ncov, hipStream_t s,
                         const Args&... args) {
    for (uint32_t level = depth; level-- > first;) {
        const uint32_t gx = (uint32_t)(((1ull << level) + kBlock - 1) / kBlock);
        for (uint32_t o0 = 0; o0 < ncov; o0 += 65535u) {
            pass<<<dim3(gx, std::min(ncov - o0, 65535u)), kBlock, 0, s>>>(level, o0, args...);
            TRY(hipGetLastError());
        }
    }
    return hipSuccess;
}

// The workgroups of 256 faces that cover a layout's objects (margin_kernel's grid).
uint32_t layout_blocks(const std::vector<DevObj>& objs) { return objs.back().block_begin + (objs.back().faces + kBlock - 1) / kBlock; }

// A refit's scratch for a layout: the uploaded layout, the accumulators and counters, per face the
// flag and (alpha, beta), per node the double bounds (no node without a culled face).
// reserve_refit_scratch lays it out in an arena — the call's own (accel_refit_device) or the one
// that becomes the persistent workspace (accel_refit_workspace) — and records the offsets in ws;
// refit_scratch gives the typed pointers for an allocation at `base`.
void reserve_refit_scratch(Arena& a, const std::vector<DevObj>& objs, size_t node_count, RefitWorkspace& ws) {
    const size_t ncov = objs.size(), F = objs.back().gbegin + objs.back().faces;
    ws.o_objs = a.reserve(sizeof(DevObj) * ncov);
    ws.o_acc = a.reserve(sizeof(DevAcc) * ncov);
    ws.o_cnt = a.reserve(sizeof(DevCount) * ncov);
    ws.o_flags = a.reserve(4 * F);
    ws.o_ab = a.reserve(16 * F);
    ws.o_bounds = a.reserve(sizeof(accel::NodeBounds) * node_count);
}

struct RefitScratch {
    DevObj* objs;
    DevAcc* acc;
    DevCount* cnt;
    uint32_t* flags;
    double* ab;
    accel::NodeBounds* bounds;
};
RefitScratch refit_scratch(const RefitWorkspace& ws, unsigned char* base) {
    return RefitScratch{reinterpret_cast<DevObj*>(base + ws.o_objs),     reinterpret_cast<DevAcc*>(base + ws.o_acc),
                        reinterpret_cast<DevCount*>(base + ws.o_cnt),    reinterpret_cast<uint32_t*>(base + ws.o_flags),
                        reinterpret_cast<double*>(base + ws.o_ab),       reinterpret_cast<accel::NodeBounds*>(base + ws.o_bounds)};
}

}  // namespace

hipError_t accel_build_device(const TriHot* d_hot, const std::vector<AccelDevObject>& covered, size_t nobj, RayAccel& ra,
                              hipStream_t s, AccelDevInfo* info, const char** refuse) {
    *refuse = nullptr;
    *info = AccelDevInfo{};
    ra.drop();
    const uint32_t ncov = (uint32_t)covered.size();
    if (!ncov) return hipSuccess;
    // (the host build's limits: at most 0x7fffffff slots here, its bound on the nodes below)
    std::vector<DevObj> objs(ncov);
    uint64_t F64 = 0, blocks64 = 0;
    for (uint32_t i = 0; i < ncov; ++i) {
        if (F64 + covered[i].faces > 0x7fffffffull) {
            *refuse = "too many nodes";
            return hipSuccess;
        }
        objs[i] = DevObj{covered[i].hot_begin, covered[i].faces, (uint32_t)F64, (uint32_t)blocks64, covered[i].index, 0, 0, 0, 0, 0, 0, 0};
        F64 += covered[i].faces;
        blocks64 += (covered[i].faces + kBlock - 1) / kBlock;
    }
    const uint32_t F = (uint32_t)F64, blocks = (uint32_t)blocks64;

    TRY(ra.objs.alloc(nobj));
    TRY(ra.hot.alloc(std::max<uint32_t>(F, 1)));
    TRY(ra.index.alloc(std::max<uint32_t>(F, 1)));
    TRY(hipMemsetAsync(ra.objs, 0, sizeof(accel::Object) * nobj, s));

    size_t scan_temp = 0;
    TRY(rocprim::exclusive_scan(nullptr, scan_temp, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)F, rocprim::plus<uint32_t>(), s));
    Arena a;
    const size_t o_objs = a.reserve(sizeof(DevObj) * ncov), o_acc = a.reserve(sizeof(DevAcc) * ncov),
                 o_cnt = a.reserve(sizeof(DevCount) * ncov), o_flags = a.reserve(4 * (size_t)F),
                 o_scan = a.reserve(4 * (size_t)F), o_ab = a.reserve(16 * (size_t)F), o_keys = a.reserve(8 * (size_t)F),
                 o_keys2 = a.reserve(8 * (size_t)F), o_ids = a.reserve(4 * (size_t)F), o_ids2 = a.reserve(4 * (size_t)F),
                 o_tmp = a.reserve(scan_temp);
    TRY(a.alloc());
    DevObj* d_objs = a.at<DevObj>(o_objs);
    DevAcc* d_acc = a.at<DevAcc>(o_acc);
    DevCount* d_cnt = a.at<DevCount>(o_cnt);
    uint32_t *d_flags = a.at<uint32_t>(o_flags), *d_scan = a.at<uint32_t>(o_scan);
    double* d_ab = a.at<double>(o_ab);
    unsigned long long *d_keys = a.at<unsigned long long>(o_keys), *d_keys2 = a.at<unsigned long long>(o_keys2);
    uint32_t *d_ids = a.at<uint32_t>(o_ids), *d_ids2 = a.at<uint32_t>(o_ids2);

    const std::vector<DevAcc> acc0(ncov, dev_acc_start());
    TRY(hipMemcpyAsync(d_objs, objs.data(), sizeof(DevObj) * ncov, hipMemcpyHostToDevice, s));
    TRY(hipMemcpyAsync(d_acc, acc0.data(), sizeof(DevAcc) * ncov, hipMemcpyHostToDevice, s));
    TRY(hipMemsetAsync(d_cnt, 0, sizeof(DevCount) * ncov, s));
    if (blocks) {
        margin_kernel<<<blocks, kBlock, 0, s>>>(d_hot, d_objs, ncov, d_flags, reinterpret_cast<double2*>(d_ab), d_acc, d_cnt);
        TRY(hipGetLastError());
        TRY(rocprim::exclusive_scan(a.at<void>(o_tmp), scan_temp, d_flags, d_scan, 0u, (size_t)F, rocprim::plus<uint32_t>(), s));
        key_kernel<<<blocks, kBlock, 0, s>>>(d_hot, d_objs, ncov, d_flags, d_scan, d_acc, d_keys, d_ids, ra.hot, ra.index);
        TRY(hipGetLastError());
    }
    // the one round trip: 16 B of counters per covered object
    std::vector<DevCount> cnt(ncov);
    TRY(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(DevCount) * ncov, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));

    uint64_t nodes = 0, P = 0;
    uint32_t depth = 0;
    for (uint32_t i = 0; i < ncov; ++i) {
        if (cnt[i].status || (uint64_t)cnt[i].culled + cnt[i].unculled != objs[i].faces) {
            *refuse = "the device builder's counters do not add up";
            ra.drop();
            return hipSuccess;
        }
        const accel::TreeLayout t = accel::tree_layout(cnt[i].culled);
        if (nodes + 2 * (uint64_t)objs[i].faces > 0x7fffffffull) {
            *refuse = "too many nodes";
            ra.drop();
            return hipSuccess;
        }
        if (t.depth > accel::kStackDepth) {
            *refuse = "the hierarchy would be deeper than the traversal stack";
            ra.drop();
            return hipSuccess;
        }
        objs[i].C = cnt[i].culled;
        objs[i].U = cnt[i].unculled;
        objs[i].cbase = (uint32_t)P;
        objs[i].node_base = (uint32_t)nodes;
        objs[i].full = t.full;
        objs[i].extra = t.extra;
        nodes += t.nodes;
        P += cnt[i].culled;
        depth = std::max(depth, t.depth);
        info->unculled += cnt[i].unculled;
    }
    info->nodes = nodes;
    info->max_depth = depth;
    TRY(ra.nodes.alloc(std::max<uint64_t>(nodes, 1)));
    if (P) {
        const uint32_t ord_bits = ncov > 1 ? 32u - (uint32_t)__builtin_clz(ncov - 1) : 0u;
        size_t sort_temp = 0, sort2_temp = 0;
        TRY(rocprim::radix_sort_pairs(nullptr, sort_temp, d_keys, d_keys2, d_ids, d_ids2, (size_t)P, 0u, 63u, s));
        if (ord_bits)
            TRY(rocprim::radix_sort_pairs(nullptr, sort2_temp, (uint32_t*)nullptr, (uint32_t*)nullptr, d_ids2, d_ids, (size_t)P, 0u,
                                          ord_bits, s));
        Arena b;
        const size_t o_bounds = b.reserve(sizeof(accel::NodeBounds) * nodes), o_sort = b.reserve(std::max(sort_temp, sort2_temp));
        TRY(b.alloc());
        accel::NodeBounds* d_bounds = b.at<accel::NodeBounds>(o_bounds);
        TRY(hipMemcpyAsync(d_objs, objs.data(), sizeof(DevObj) * ncov, hipMemcpyHostToDevice, s));
        TRY(rocprim::radix_sort_pairs(b.at<void>(o_sort), sort_temp, d_keys, d_keys2, d_ids, d_ids2, (size_t)P, 0u, 63u, s));
        const uint32_t* sorted = d_ids2;
        if (ord_bits) {  // (the flag and scan arrays are free now: the ordinals and their sorted copy)
            ordinal_kernel<<<(uint32_t)((P + kBlock - 1) / kBlock), kBlock, 0, s>>>(d_objs, ncov, d_ids2, (uint32_t)P, d_flags);
            TRY(hipGetLastError());
            TRY(rocprim::radix_sort_pairs(b.at<void>(o_sort), sort2_temp, d_flags, d_scan, d_ids2, d_ids, (size_t)P, 0u, ord_bits, s));
            sorted = d_ids;
        }
        TRY(launch_levels(level_kernel, 0u, depth, ncov, s, d_hot, d_objs, sorted, d_ab, ra.nodes, d_bounds, ra.hot, ra.index));
        object_kernel<<<(ncov + kBlock - 1) / kBlock, kBlock, 0, s>>>(d_objs, ncov, d_acc, ra.objs);
        TRY(hipGetLastError());
        TRY(hipStreamSynchronize(s));  // (the temporaries go out of scope)
    } else {
        TRY(hipMemcpyAsync(d_objs, objs.data(), sizeof(DevObj) * ncov, hipMemcpyHostToDevice, s));
        object_kernel<<<(ncov + kBlock - 1) / kBlock, kBlock, 0, s>>>(d_objs, ncov, d_acc, ra.objs);
        TRY(hipGetLastError());
        TRY(hipStreamSynchronize(s));
    }
    ra.layout = objs;  // (the refit's: accel_refit_device)
    ra.max_depth = depth;
    return hipSuccess;
}

hipError_t accel_refit_device(const TriHot* d_hot, RayAccel& ra, hipStream_t s, AccelDevInfo* info, bool* kept) {
    *info = AccelDevInfo{};
    *kept = false;
    const std::vector<DevObj>& objs = ra.layout;
    const uint32_t ncov = (uint32_t)objs.size();
    if (!ncov) return hipSuccess;
    const uint32_t blocks = layout_blocks(objs);
    Arena a;
    RefitWorkspace at;  // (the offsets only: the arena keeps the memory)
    reserve_refit_scratch(a, objs, ra.node_count, at);
    TRY(a.alloc());
    const RefitScratch w = refit_scratch(at, a.mem);

    const std::vector<DevAcc> acc0(ncov, dev_acc_start());
    TRY(hipMemcpyAsync(w.objs, objs.data(), sizeof(DevObj) * ncov, hipMemcpyHostToDevice, s));
    TRY(hipMemcpyAsync(w.acc, acc0.data(), sizeof(DevAcc) * ncov, hipMemcpyHostToDevice, s));
    TRY(hipMemsetAsync(w.cnt, 0, sizeof(DevCount) * ncov, s));
    if (blocks) {
        margin_kernel<<<blocks, kBlock, 0, s>>>(d_hot, w.objs, ncov, w.flags, reinterpret_cast<double2*>(w.ab), w.acc, w.cnt);
        TRY(hipGetLastError());
        refit_check_kernel<<<blocks, kBlock, 0, s>>>(d_hot, w.objs, ncov, w.flags, ra.index, ra.hot, w.cnt);
        TRY(hipGetLastError());
    }
    // the one round trip, the build's: 16 B of counters per covered object
    std::vector<DevCount> cnt(ncov);
    TRY(hipMemcpyAsync(cnt.data(), w.cnt, sizeof(DevCount) * ncov, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < ncov; ++i) {
        if (cnt[i].status || cnt[i].culled != objs[i].C || cnt[i].unculled != objs[i].U) return hipSuccess;  // a class change
        info->unculled += objs[i].U;
    }
    info->nodes = ra.node_count;
    info->max_depth = ra.max_depth;
    if (ra.node_count)
        TRY(launch_levels(preorder(objs) ? refit_level_preorder_kernel : refit_level_kernel, 0u, ra.max_depth, ncov, s, d_hot, w.objs,
                          w.ab, ra.nodes, w.bounds, ra.hot, ra.index));
    object_kernel<<<(ncov + kBlock - 1) / kBlock, kBlock, 0, s>>>(w.objs, ncov, w.acc, ra.objs);
    TRY(hipGetLastError());
    TRY(hipStreamSynchronize(s));  // (the temporaries go out of scope)
    *kept = true;
    return hipSuccess;
}

hipError_t accel_refit_workspace(RayAccel& ra, hipStream_t s) {
    RefitWorkspace& ws = ra.refit;
    ws.release();
    const std::vector<DevObj>& objs = ra.layout;
    const uint32_t ncov = (uint32_t)objs.size();
    if (!ncov) return hipSuccess;
    uint32_t max_full = 0;
    for (const DevObj& ob : objs)
        if (ob.C) max_full = std::max(max_full, ob.full);
    Arena a;
    reserve_refit_scratch(a, objs, ra.node_count, ws);
    ws.o_verdict = a.reserve(4 * (size_t)ncov);
    ws.o_refits = a.reserve(4);
    TRY(a.alloc());
    // nothing has run yet: zero refits, and every covered object is searched through the build's tree
    const std::vector<uint32_t> ones(ncov, 1u);
    TRY(hipMemsetAsync(a.at<void>(0), 0, std::max<size_t>(a.need, 256), s));
    TRY(hipMemcpyAsync(a.at<DevObj>(ws.o_objs), objs.data(), sizeof(DevObj) * ncov, hipMemcpyHostToDevice, s));
    TRY(hipMemcpyAsync(a.at<uint32_t>(ws.o_verdict), ones.data(), 4 * (size_t)ncov, hipMemcpyHostToDevice, s));
    TRY(hipStreamSynchronize(s));  // (the uploads' sources are this call's)
    ws.bytes = std::max<size_t>(a.need, 256);
    ws.ncov = ncov;
    ws.blocks = layout_blocks(objs);
    ws.first_deep = accel::refit_first_deep(max_full);
    ws.mem = std::move(a.mem);
    return hipSuccess;
}

// Memory safety of the level passes whatever the faces hold (they run before the verdict is known
// to anyone): level_node takes every range from the layout (node_range: C, full, extra) and every
// node id from its numbering (LevelOrder: node_id, first_child; PreOrder: id, subtree_nodes — both
// arithmetic on C, the level and the lane, below the tree's node count, which the build's node array
// holds from node_base on), make_leaf indexes faces / alpha_beta by entries of the index array — which
// the build filled with the object's face indices and which a refit only permutes inside leaf ranges
// — and stores to slots and node ids computed from the layout; make_inner reads two node ids computed
// from the layout.  No face value (NaN, infinite, huge) reaches an index: such values end in boxes
// and margins of an object whose record then says has = 0.  A host-built tree qualifies on the same
// terms: accel_build.cpp's build_scene records its layout only after checking that its node count and
// depth are tree_layout(C)'s (fits_tree_layout).
hipError_t accel_refit_enqueue(const TriHot* d_hot, RayAccel& ra, hipStream_t s) {
    const RefitWorkspace& ws = ra.refit;
    const uint32_t ncov = ws.ncov;
    if (!ws.ready() || !ncov) return hipSuccess;
    unsigned char* base = ws.mem;
    const RefitScratch w = refit_scratch(ws, base);
    const uint32_t og = (ncov + kBlock - 1) / kBlock;
    refit_reset_kernel<<<og, kBlock, 0, s>>>(w.acc, w.cnt, ncov);
    TRY(hipGetLastError());
    if (ws.blocks) {
        margin_kernel<<<ws.blocks, kBlock, 0, s>>>(d_hot, w.objs, ncov, w.flags, reinterpret_cast<double2*>(w.ab), w.acc, w.cnt);
        TRY(hipGetLastError());
        refit_check_kernel<<<ws.blocks, kBlock, 0, s>>>(d_hot, w.objs, ncov, w.flags, ra.index, ra.hot, w.cnt);
        TRY(hipGetLastError());
    }
    if (ra.node_count) {
        const uint32_t first_deep = ra.refit_top_levels ? ws.first_deep : 0u;
        const bool pre = preorder(ra.layout);
        const auto top_pass = pre ? refit_top_levels_preorder_kernel : refit_top_levels_kernel;
        TRY(launch_levels(pre ? refit_level_preorder_kernel : refit_level_kernel, first_deep, ra.max_depth, ncov, s, d_hot, w.objs, w.ab,
                          ra.nodes, w.bounds, ra.hot, ra.index));
        if (first_deep) {
            top_pass<<<ncov, kBlock, 0, s>>>(std::min(first_deep, ra.max_depth), 0u, d_hot, w.objs, w.ab, ra.nodes, w.bounds, ra.hot,
                                             ra.index);
            TRY(hipGetLastError());
        }
    }
    refit_object_kernel<<<og, kBlock, 0, s>>>(w.objs, ncov, w.acc, w.cnt, ra.objs, reinterpret_cast<uint32_t*>(base + ws.o_verdict),
                                              reinterpret_cast<uint32_t*>(base + ws.o_refits));
    return hipGetLastError();
}

hipError_t accel_refit_status(const RayAccel& ra, hipStream_t s, uint32_t* refits, uint32_t* kept) {
    const RefitWorkspace& ws = ra.refit;
    *refits = *kept = 0;
    if (!ws.ready()) return hipSuccess;
    unsigned char* base = ws.mem;
    std::vector<uint32_t> verdict(ws.ncov);
    TRY(hipStreamSynchronize(s));
    TRY(hipMemcpy(verdict.data(), base + ws.o_verdict, 4 * (size_t)ws.ncov, hipMemcpyDeviceToHost));
    TRY(hipMemcpy(refits, base + ws.o_refits, 4, hipMemcpyDeviceToHost));
    for (uint32_t v : verdict) *kept += v ? 1u : 0u;
    return hipSuccess;
}

}  // namespace gpu
}  // namespace eray
