// pt_trace.h -- device code shared by the kernel translation units: the opening of every kernel that walks the tree (stage_scene,
// tree_walk_setup), BVH traversal (closest_hit, wide_visit, primary-beam helpers), the shading step of the bounce loop (shade_step:
// Raytracing.hlsl:213-364) and the fused trace + shade kernel bounce_kernel with its launcher template (over pt_launch.h).
// pt_kernels.hip holds the other kernels; pt_bounce_*.hip instantiate bounce_kernel for one (BVH residence, stack entry type) pair
// each, so that the ~100 instances compile in parallel.
//
// Everything is compiled with -ffp-contract=off; arithmetic that decides a branch follows pt_math.h /
// pt_bsdf.h (bit-exact with the CPU oracle).  The AABB slab test is traversal-only arithmetic: it must be
// conservative, not bit-reproducible on the CPU (DESIGN.md "LBVH").
#pragma once

#include "pt_kernels.h"
#include "pt_launch.h"
#include "pt_beam.h"

namespace pt {

// ------------------------------------------------------------------------------------------------ helpers
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// Reciprocal of a ray-direction component for the slab test t = fma(plane, inv, -o * inv).  A zero (or denormal-tiny)
// component would give inv = inf and then inf - inf = NaN for the planes on one side of the origin, and fmax(-inf, NaN)
// = -inf would wrongly close the slab: the component is replaced by +-`tiny` (SceneView::slab_tiny).  In a scene whose
// coordinates stay below 1e8 that is 1e-30, which keeps -o * inv finite for every origin between two planes and makes the
// slab interval (-huge, +huge) when the origin lies between the planes and empty otherwise -- the exact behaviour of an
// axis-parallel ray.  Found by tests/test_gpu_fuzz.py (centre column of an odd-width frame with zero jitter: d.x == 0).
// In a larger scene -o * 1e30 (and the wide walk's cell * 1e30) would overflow to an infinity of ONE sign for both planes
// of a slab that holds the origin and close it; there `tiny` is NaN, every ray parameter of that axis is NaN, and the
// min / max of the slab test drop them: the axis does not cull, which is conservative.  Found by tests/test_gpu_wide.py
// (`geometric`: coordinates up to 1e25).
__device__ __forceinline__ float slab_rcp(float d, float tiny)
{
    return fast_rcp(__builtin_fabsf(d) < 1e-30f ? __builtin_copysignf(tiny, d) : d);
}

// Adds the sum of `v` over the workgroup to *counter with ONE atomic (wave shuffle -> LDS -> thread 0).  Same-address
// device-scope atomics from all 8 XCDs serialise; one per wave has been measured to dominate short kernels.
__device__ __forceinline__ void block_atomic_add(unsigned long long* counter, unsigned long long v)
{
    __shared__ unsigned long long s_part[16];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (uint32_t w = 0; w < (blockDim.x + 63u) / 64u; w++) sum += s_part[w];
        if (sum) atomicAdd(counter, sum);
    }
}

// Called by every thread of ONE block: fold a finished frame's counters (queue sizes 1..n + its tail counter) into
// the running totals and leave them zeroed.
__device__ __forceinline__ void fold_counters(uint32_t* __restrict__ counts, uint32_t n_counts, unsigned long long* __restrict__ tail,
                                              unsigned long long* __restrict__ totals, uint32_t* __restrict__ host_counts)
{
    __shared__ unsigned long long s_sum[16];
    unsigned long long s = 0;
    for (uint32_t k = 1 + threadIdx.x; k <= n_counts; k += blockDim.x) s += counts[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63u) == 0) s_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = *tail;
        for (uint32_t w = 0; w < (blockDim.x + 63u) / 64u; w++) t += s_sum[w];
        totals[0] += t;
        totals[1] = t;
        *tail = 0ull;
    }
    __syncthreads();
    // publish the folded frame's queue sizes to the host (it sizes later frames' grids from them); counts[0] == 0 means
    // these counters hold no frame (already folded)
    if (host_counts && counts[0] != 0u)
        for (uint32_t k = threadIdx.x; k <= n_counts; k += blockDim.x) host_counts[k] = counts[k];
    for (uint32_t k = threadIdx.x; k < 2u * (n_counts + 1u); k += blockDim.x) counts[k] = 0u;  // queue sizes + work cursors
}

// First kernel of a frame, block 0: fold the previous frame (other parity), publish this frame's queue-0 size.
// This frame's counters were zeroed when the frame before the previous one was folded (or at allocation).
__device__ __forceinline__ void frame_counters_begin(const FrameCounters& fc, uint32_t n_slots)
{
    fold_counters(fc.fold_counts, fc.n_counts, fc.fold_tail, fc.totals, fc.host_counts);
    if (threadIdx.x == 0) fc.counts[0] = n_slots;
}

// Stage the BVH (nodes, Morton-ordered spheres, ids) into LDS.  Layout: [nodes | spheres | ids].
// (sync = false: the caller has more to put in LDS before the barrier, and makes it itself)
__device__ __forceinline__ void stage_scene(const SceneView& sv, float4* lds, bool sync = true)
{
    const uint32_t n_vec = sv.n_nodes * 4u + sv.n;
    for (uint32_t i = threadIdx.x; i < n_vec; i += blockDim.x)
        lds[i] = i < sv.n_nodes * 4u ? sv.nodes[i] : sv.sph_sorted[i - sv.n_nodes * 4u];
    uint32_t* ids = reinterpret_cast<uint32_t*>(lds + n_vec);
    for (uint32_t i = threadIdx.x; i < sv.n; i += blockDim.x) ids[i] = sv.sorted_id[i];
    if (sync) __syncthreads();
}

__host__ __device__ inline uint32_t scene_lds_bytes(uint32_t n_nodes, uint32_t n) { return (n_nodes * 4u + n) * 16u + ((n * 4u + 15u) & ~15u); }

// What a lane walks the tree with: the tree as the walkers read it and the lane's stack (entry k at stack[k * blockDim.x]).
template <typename StackT>
struct TreeWalk {
    const float4* nodes;
    const float4* sph;
    const uint32_t* ids;
    StackT* stack;
};

// Fills `w`.  (By reference on purpose: with the struct returned by value the kernels' register allocation moves -- scratch bytes
// of a bounce_kernel instance, SGPR spills of several side-pass instances; profiles/n20_isa_*.)  kLds: the copy stage_scene has made or is making at the start of the dynamic LDS (nothing is read here), the stacks
// behind it; else the tree in global memory, the stacks at the start of the dynamic LDS.
template <bool kLds, typename StackT>
__device__ __forceinline__ void tree_walk_pointers(const SceneView& sv, TreeWalk<StackT>& w)
{
    extern __shared__ float4 smem[];
    if (kLds) {
        w.nodes = smem;
        w.sph = smem + sv.n_nodes * 4u;
        w.ids = reinterpret_cast<const uint32_t*>(smem + sv.n_nodes * 4u + sv.n);
        w.stack = reinterpret_cast<StackT*>(reinterpret_cast<char*>(smem) + scene_lds_bytes(sv.n_nodes, sv.n));
    } else {
        w.nodes = sv.nodes;
        w.sph = sv.sph_sorted;
        w.ids = sv.sorted_id;
        w.stack = reinterpret_cast<StackT*>(smem);
    }
    w.stack += threadIdx.x;
}

// The opening of a kernel that walks the tree, called by every thread of the workgroup (kLds: staging ends with a barrier).
template <bool kLds, typename StackT>
__device__ __forceinline__ void tree_walk_setup(const SceneView& sv, TreeWalk<StackT>& w)
{
    extern __shared__ float4 smem[];
    if (kLds) stage_scene(sv, smem);
    tree_walk_pointers<kLds, StackT>(sv, w);
}

// Stack entries hold a child reference: internal node index i >= 0, or leaf (Morton-sorted sphere index k) as ~k.
// The 16-bit stack (trees with < 32768 leaves) stores a leaf as 0x8000 | k.
template <typename StackT> __device__ __forceinline__ StackT stack_encode(int c);
template <> __device__ __forceinline__ uint16_t stack_encode<uint16_t>(int c) { return c < 0 ? (uint16_t)(0x8000u | (uint32_t)~c) : (uint16_t)c; }
template <> __device__ __forceinline__ uint32_t stack_encode<uint32_t>(int c) { return (uint32_t)c; }
__device__ __forceinline__ int stack_decode(uint16_t v) { return (v & 0x8000u) ? ~(int)(v & 0x7FFFu) : (int)v; }
__device__ __forceinline__ int stack_decode(uint32_t v) { return (int)v; }

constexpr int kTraversalDone = (int)0x80000000;  // not a valid leaf code (leaf codes are >= -2^30)

// fminf / fmaxf against a value the compiler cannot prove quiet (tmin and the running best cross basic blocks) cost an extra
// v_max x, x per operand and per node visit.  Neither is ever a signalling NaN, so the slab test names the instruction itself:
// v_min_f32 / v_max_f32 return the other operand for a quiet NaN exactly as fminf / fmaxf do ("Conservativeness").  Measured: C2 -0.8 %.
__device__ __forceinline__ float raw_minf(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float raw_maxf(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// One visit of a 4-wide node (pt_lbvh_gpu.hip collapse4_kernel: the grandchildren of an even-depth binary node, their boxes as
// 8-bit offsets on a per-node power-of-two grid; global-memory scenes): four slab tests from ONE 64-byte record, the hit
// children ordered near to far by a 5-exchange network, the nearest descended into, the others pushed far-first.  Half the
// dependent fetches AND half the sectors per ray of the binary walk (DESIGN.md "Wide nodes").  A plane's ray parameter is
// t = fma(byte, cell * (1/d), fma(origin, 1/d, -o/d)): the decode fma(byte, cell, origin) folded into the slab test.
// Sets node = kTraversalDone when nothing is left.
template <typename StackT>
__device__ __forceinline__ void wide_visit(const float4* __restrict__ wide, int& node, uint32_t& sp, StackT* stack, uint32_t stride, float ix, float iy,
                                           float iz, float ox, float oy, float oz, float tmin, float best)
{
    const uint4* __restrict__ w = reinterpret_cast<const uint4*>(wide) + (size_t)node * 4u;
    const uint4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    const float sx = as_float((w0.w & 0xFFu) << 23) * ix, sy = as_float(((w0.w >> 8) & 0xFFu) << 23) * iy, sz = as_float(((w0.w >> 16) & 0xFFu) << 23) * iz;
    const float bx0 = pt_fma(as_float(w0.x), ix, ox), by0 = pt_fma(as_float(w0.y), iy, oy), bz0 = pt_fma(as_float(w0.z), iz, oz);
    float tn[4];
    int ref[4] = { (int)w2.z, (int)w2.w, (int)w3.x, (int)w3.y };
#define PT_WIDE_CHILD(c)                                                                                                 \
    {                                                                                                                    \
        const float ax = pt_fma((float)((w1.x >> (8 * c)) & 0xFFu), sx, bx0), bx = pt_fma((float)((w1.w >> (8 * c)) & 0xFFu), sx, bx0);   \
        const float ay = pt_fma((float)((w1.y >> (8 * c)) & 0xFFu), sy, by0), by = pt_fma((float)((w2.x >> (8 * c)) & 0xFFu), sy, by0);   \
        const float az = pt_fma((float)((w1.z >> (8 * c)) & 0xFFu), sz, bz0), bz = pt_fma((float)((w2.y >> (8 * c)) & 0xFFu), sz, bz0);   \
        const float tnear = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), raw_maxf(fminf(az, bz), tmin));                   \
        const float tfar = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), raw_minf(fmaxf(az, bz), best));                    \
        tn[c] = (tnear <= tfar && ref[c] != kTraversalDone) ? tnear : kInf;                                             \
    }
    PT_WIDE_CHILD(0) PT_WIDE_CHILD(1) PT_WIDE_CHILD(2) PT_WIDE_CHILD(3)
#undef PT_WIDE_CHILD
#define PT_WIDE_CSWAP(a, b)                                                                                              \
    {                                                                                                                    \
        const bool sw = tn[b] < tn[a];                                                                                   \
        const float ta = sw ? tn[b] : tn[a], tb = sw ? tn[a] : tn[b];                                                    \
        const int ra = sw ? ref[b] : ref[a], rb = sw ? ref[a] : ref[b];                                                  \
        tn[a] = ta; tn[b] = tb; ref[a] = ra; ref[b] = rb;                                                                \
    }
    PT_WIDE_CSWAP(0, 1) PT_WIDE_CSWAP(2, 3) PT_WIDE_CSWAP(0, 2) PT_WIDE_CSWAP(1, 3) PT_WIDE_CSWAP(1, 2)
#undef PT_WIDE_CSWAP
    if (tn[3] < kInf) { stack[sp] = stack_encode<StackT>(ref[3]); sp += stride; }
    if (tn[2] < kInf) { stack[sp] = stack_encode<StackT>(ref[2]); sp += stride; }
    if (tn[1] < kInf) { stack[sp] = stack_encode<StackT>(ref[1]); sp += stride; }
    if (tn[0] < kInf) {
        node = ref[0];
    } else if (sp == 0) {
        node = kTraversalDone;
    } else {
        sp -= stride;
        node = stack_decode(stack[sp]);
    }
}

// ------------------------------------------------------------------------------------------------ alpha-tested hits (spec S10)
// IsOpaque (ShadingHelpers.hlsli:105-115) for the crossing at parameter t of a kAlphaTested sphere: alpha = BaseColor.a * the
// base-colour map's alpha at the crossing's texture coordinates (the class says EvaluateBaseColor samples, :61-72); accepted iff
// alpha >= AlphaCutoff.  Out of line (plain pointers, nothing of the kernel's argument structs): a rare path that the traversal loops
// of every textured kernel would otherwise carry several inlined copies of -- those kernels are bound by their code size as it is.
__device__ __attribute__((noinline)) inline bool crossing_is_opaque_ptr(const float4* __restrict__ mats, const uint32_t* __restrict__ tex_maps, const TexView* __restrict__ tex,
                                                                        const float4* __restrict__ rot, uint32_t id, f3 C, f3 o, f3 d, float t)
{
    const float base_alpha = mats[id * 4 + 0].w, cutoff = mats[id * 4 + 3].y;
    const uint32_t map = tex_maps[(size_t)id * 8u + kMapBaseColor];
    const f3 N = normalize(mad(t, d, o) - C);  // the hit frame's normal
    float4 q;
    f3 n_mesh;
    const f2 uv = hit_uv_rot(rot, id, N, q, n_mesh);
    float s[4];
    sample_bilinear(tex[map], uv, s);
    return base_alpha * s[3] >= cutoff;
}
__device__ __forceinline__ bool crossing_is_opaque(const SceneView& sv, uint32_t id, f3 C, f3 o, f3 d, float t)
{
    return crossing_is_opaque_ptr(sv.mats, sv.tex_maps, sv.tex, sv.rot, id, C, o, d, t);
}

// A sphere test succeeded at t for the leaf with flagged id `idf` whose class bits are set (rare): does the sphere offer an
// accepted crossing?  kAlphaInvisible: never.  kAlphaTested: the crossing at t, else the one behind it ("the next crossing" =
// intersect_sphere with tmin = the rejected t: the far root, seen from inside); t returns the accepted one.  kAlphaTex = false
// (kernels of scenes without textures, where the class cannot occur): accepted.
template <bool kAlphaTex>
__device__ __forceinline__ bool alpha_candidate(const SceneView& sv, uint32_t idf, f3 C, float r, f3 o, f3 d, float& t)
{
    if ((idf >> kIdClassShift) == kAlphaInvisible) return false;
    if (!kAlphaTex) return true;
    const uint32_t id = idf & kIdMask;
    for (;;) {
        if (crossing_is_opaque(sv, id, C, o, d, t)) return true;
        float t2;
        if (!intersect_sphere(o, d, t, kInf, C, r, t2)) return false;
        t = t2;
    }
}

// Closest hit over the LBVH ("while-while" traversal: descend internal nodes until every lane of the wave holds a
// leaf or has finished, then run the sphere tests together).  nodes/sph/ids may live in LDS or global memory (the
// address space is inferred after inlining).  stack: per-lane stack, entry e of lane l at stack[e * stride + l].
// The result is identical to brute force: nearest t, ties -> lowest original id (leaf boxes are padded so the slab
// test is conservative w.r.t. intersect_sphere; culling is <=).
// kWide: `nodes` is the 4-wide view of the tree (128-byte records, wide_visit) instead of the binary records.
// kAlphaTex: the per-crossing alpha test of kAlphaTested spheres is compiled in (alpha_candidate).
template <typename StackT, bool kCount = false, bool kWide = false, bool kAlphaTex = false>
__device__ __forceinline__ void closest_hit(const SceneView& sv, const float4* __restrict__ nodes, const float4* __restrict__ sph,
                                            const uint32_t* __restrict__ ids, uint32_t n, f3 o, f3 d, float tmin, float tmax,
                                            StackT* stack, uint32_t stride, float& t_out, uint32_t& id_out, uint32_t* visits = nullptr, uint32_t descent_cap = 0)
{
    uint32_t n_nodes_visited = 0, n_spheres_tested = 0;  // kCount only (pt_trace_rays statistics hook)
    float best = tmax;
    uint32_t best_id = kMissId;
    if (n == 1) {
        float4 s = sph[0];
        float t;
        if (intersect_sphere(o, d, tmin, kInf, make_f3(s.x, s.y, s.z), s.w, t)) {
            const uint32_t idf = ids[0];
            if ((idf >> kIdClassShift) == 0u || alpha_candidate<kAlphaTex>(sv, idf, make_f3(s.x, s.y, s.z), s.w, o, d, t))
                if (t < best) { best = t; best_id = idf & kIdMask; }
        }
        t_out = best; id_out = best_id;
        return;
    }
    const float ix = slab_rcp(d.x, sv.slab_tiny), iy = slab_rcp(d.y, sv.slab_tiny), iz = slab_rcp(d.z, sv.slab_tiny);
    const float ox = -o.x * ix, oy = -o.y * iy, oz = -o.z * iz;
    int node = 0;
    uint32_t sp = 0;  // stack offset in elements: a multiple of `stride` (entry e of this lane lives at stack[e * stride])
    for (;;) {
        // descent_cap > 0 bounds the node visits a lane makes before the wave turns to the sphere tests (incoherent rays in big
        // scenes: lanes that already hold a leaf otherwise idle until the longest descent of the wave ends); 0 = unbounded
        uint32_t budget = descent_cap;
        while (node >= 0) {
            if (kCount) n_nodes_visited++;
            if (kWide) { wide_visit<StackT>(nodes, node, sp, stack, stride, ix, iy, iz, ox, oy, oz, tmin, best); if (--budget == 0u) break; continue; }
            const float4 n0 = nodes[node * 4 + 0];
            const float4 n1 = nodes[node * 4 + 1];
            const float4 n2 = nodes[node * 4 + 2];
            const float4 n3 = nodes[node * 4 + 3];
            // child 0: lo = (n0.x,n0.y,n0.z) hi = (n0.w,n1.x,n1.y); child 1: lo = (n1.z,n1.w,n2.x) hi = (n2.y,n2.z,n2.w)
            // A min / max costs a whole 4-cycle slot unless its neighbour is an fma (tools/experiments/int_rate.hip, profiles/r02_valu_mix.txt):
            // child 1's plane distances are written between child 0's min / max (the scheduler has the last word; it made no measurable difference).
            const float ax = pt_fma(n0.x, ix, ox), bx = pt_fma(n0.w, ix, ox);
            const float ay = pt_fma(n0.y, iy, oy), by = pt_fma(n1.x, iy, oy);
            const float az = pt_fma(n0.z, iz, oz), bz = pt_fma(n1.y, iz, oz);
            const float lx0 = fminf(ax, bx); const float cx = pt_fma(n1.z, ix, ox);
            const float ly0 = fminf(ay, by); const float dx = pt_fma(n2.y, ix, ox);
            const float lz0 = fminf(az, bz); const float cy = pt_fma(n1.w, iy, oy);
            const float hx0 = fmaxf(ax, bx); const float dy = pt_fma(n2.z, iy, oy);
            const float hy0 = fmaxf(ay, by); const float cz = pt_fma(n2.x, iz, oz);
            const float hz0 = fmaxf(az, bz); const float dz = pt_fma(n2.w, iz, oz);
            const float tn0 = fmaxf(fmaxf(lx0, ly0), raw_maxf(lz0, tmin));
            const float tf0 = fminf(fminf(hx0, hy0), raw_minf(hz0, best));
            const float tn1 = fmaxf(fmaxf(fminf(cx, dx), fminf(cy, dy)), raw_maxf(fminf(cz, dz), tmin));
            const float tf1 = fminf(fminf(fmaxf(cx, dx), fmaxf(cy, dy)), raw_minf(fmaxf(cz, dz), best));
            const bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
            const int c0 = __builtin_bit_cast(int, n3.x), c1 = __builtin_bit_cast(int, n3.y);
            if (h0 && h1) {
                const bool swap = tn1 < tn0;
                const int near_c = swap ? c1 : c0, far_c = swap ? c0 : c1;
                stack[sp] = stack_encode<StackT>(far_c);
                sp += stride;
                node = near_c;
            } else if (h0) {
                node = c0;
            } else if (h1) {
                node = c1;
            } else if (sp == 0) {
                node = kTraversalDone;
            } else {
                sp -= stride;
                node = stack_decode(stack[sp]);
            }
            if (--budget == 0u) break;
        }
        if (node == kTraversalDone) break;
        if (node >= 0) continue;  // the budget ran out mid-descent
        {
            if (kCount) n_spheres_tested++;
            const uint32_t k = ~(uint32_t)node;
            const float4 s = sph[k];
            float t;
            if (intersect_sphere(o, d, tmin, kInf, make_f3(s.x, s.y, s.z), s.w, t)) {
                const uint32_t idf = ids[k];
                if ((idf >> kIdClassShift) == 0u || alpha_candidate<kAlphaTex>(sv, idf, make_f3(s.x, s.y, s.z), s.w, o, d, t)) {
                    const uint32_t id = idf & kIdMask;
                    if (t < best || (t == best && best_id != kMissId && id < best_id)) { best = t; best_id = id; }
                }
            }
        }
        if (sp == 0) break;
        sp -= stride;
        node = stack_decode(stack[sp]);
    }
    // t < tmax is required by intersect_sphere's contract: best starts at tmax and only shrinks
    t_out = best; id_out = best_id;
    if (kCount && visits) { visits[0] += n_nodes_visited; visits[1] += n_spheres_tested; }
}

// closest_hit through whichever view of the tree the scene offers: the LDS copy (binary records) when kLds, else the 4-wide view
// when the scene has one (SceneView::wide), else the binary records in global memory
template <bool kLds, typename StackT, bool kAlphaTex = false>
__device__ __forceinline__ void closest_hit_any(const SceneView& sv, const float4* __restrict__ nodes, const float4* __restrict__ sph,
                                                const uint32_t* __restrict__ ids, f3 o, f3 d, float tmin, float tmax, StackT* stack, uint32_t stride,
                                                float& t_out, uint32_t& id_out, uint32_t* visits = nullptr)
{
    // visits (global-memory scenes): this lane's running {node visits, sphere tests}, the scene term of SURVEY 8(d)'s byte accounting
    if (!kLds && visits) {
        if (sv.wide) closest_hit<StackT, true, true, kAlphaTex>(sv, sv.wide, sph, ids, sv.n, o, d, tmin, tmax, stack, stride, t_out, id_out, visits, sv.descent_cap);
        else closest_hit<StackT, true, false, kAlphaTex>(sv, nodes, sph, ids, sv.n, o, d, tmin, tmax, stack, stride, t_out, id_out, visits, sv.descent_cap);
    } else if (!kLds && sv.wide) {
        closest_hit<StackT, false, true, kAlphaTex>(sv, sv.wide, sph, ids, sv.n, o, d, tmin, tmax, stack, stride, t_out, id_out, nullptr, sv.descent_cap);
    } else {
        closest_hit<StackT, false, false, kAlphaTex>(sv, nodes, sph, ids, sv.n, o, d, tmin, tmax, stack, stride, t_out, id_out, nullptr, sv.descent_cap);
    }
}

// ------------------------------------------------------------------------------------------------ cooperative walk
// The looping pass of a 1-spp frame runs on nearly empty waves: while a few lanes walk the tree, the others idle, and the wave
// takes as long as its longest walk.  closest_hit_coop splits each live ray's walk over k = 2, 4 or 8 lanes: helper j of a ray starts at the
// j-th node of the tree's cut at depth log2 k, the helpers share the nearest hit distance found so far for culling, and their answers are
// combined by closest_hit's own rule (nearest t, ties -> lowest original id) -- a closest-hit query does not depend on the order of the
// tests, so the result is closest_hit's bit for bit.

// The cuts of the binary tree at depths 1, 2 and 3: s_cut[k - 2 + j] = start of helper j of k (a child reference, or kTraversalDone where
// a leaf above the cut has left the slot empty; kCutSlots entries).  One thread builds it, after stage_scene (n >= 2: the root is an internal node).
__device__ __forceinline__ void build_cut(const float4* __restrict__ nodes, int* s_cut)
{
    auto expand = [&](int ref, int& a, int& b) {
        if (ref >= 0) {
            const float4 n3 = nodes[ref * 4 + 3];
            a = __builtin_bit_cast(int, n3.x); b = __builtin_bit_cast(int, n3.y);
        } else {
            a = ref; b = kTraversalDone;  // a leaf keeps one slot, nothing keeps none
        }
    };
    expand(0, s_cut[0], s_cut[1]);
    for (uint32_t k = 2; k <= 4; k <<= 1)
        for (uint32_t j = 0; j < k; j++) expand(s_cut[k - 2 + j], s_cut[2 * k - 2 + 2 * j], s_cut[2 * k - 2 + 2 * j + 1]);
}

// lane l takes `v` of the lane that `ctrl` (a DPP control within a row of 16) names
template <int kCtrl> __device__ __forceinline__ uint32_t dpp_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, 0xF, 0xF, false); }
template <int kCtrl> __device__ __forceinline__ float dpp_f32(float v) { return as_float(dpp_u32<kCtrl>(as_uint(v))); }
constexpr int kDppSwap1 = 0xB1;   // quad_perm [1,0,3,2]: lane ^ 1
constexpr int kDppSwap2 = 0x4E;   // quad_perm [2,3,0,1]: lane ^ 2
constexpr int kDppMirror8 = 0x141;  // row_half_mirror: lane -> 7 - lane within 8 (the other quad)

// minimum of v over the lane's group of k consecutive lanes (k wave-uniform; every lane of the wave active)
__device__ __forceinline__ float group_min(float v, uint32_t k)
{
    v = raw_minf(v, dpp_f32<kDppSwap1>(v));
    if (k >= 4u) v = raw_minf(v, dpp_f32<kDppSwap2>(v));
    if (k >= 8u) v = raw_minf(v, dpp_f32<kDppMirror8>(v));
    return v;
}

// Closest hits of the rays of the wave's `alive` lanes (ballot = __ballot(alive), at most 32 of them, n >= 2), over the LDS-resident binary
// tree.  EVERY lane of the wave calls this, converged.  Live lane number r (in lane order) owns lanes [r * k, r * k + k) with k the largest
// of {8, 4, 2} that fits; results come back in t_out / id_out of the alive lanes only.
template <typename StackT>
__device__ __forceinline__ void closest_hit_coop(const float4* __restrict__ nodes, const float4* __restrict__ sph, const uint32_t* __restrict__ ids,
                                                 const int* __restrict__ s_cut, unsigned long long ballot, f3 o, f3 d, float tmin, float tmax,
                                                 StackT* stack, uint32_t stride, float& t_out, uint32_t& id_out, uint32_t descent_cap, float slab_tiny)
{
    const uint32_t lane = lane_id();
    const uint32_t n_live = (uint32_t)__builtin_amdgcn_readfirstlane(__popcll(ballot));
    const uint32_t shift = n_live <= 8u ? 3u : (n_live <= 16u ? 2u : 1u), k = 1u << shift;
    const uint32_t group = lane >> shift, j = lane & (k - 1u);
    // the lane of live ray number `group`: the group-th set bit of the ballot (binary search by population counts)
    uint32_t src;
    {
        const uint32_t lo = (uint32_t)ballot, hi = (uint32_t)(ballot >> 32);
        uint32_t r = group, m = lo, c = __popc(lo);
        src = 0;
        if (r >= c) { r -= c; m = hi; src = 32u; }
#pragma unroll
        for (uint32_t w = 16; w > 0; w >>= 1) {
            c = __popc(m & ((1u << w) - 1u));
            if (r >= c) { r -= c; m >>= w; src += w; }
        }
    }
    const bool has_ray = group < n_live;
    src = has_ray ? src : lane;
    const f3 ro = make_f3(__shfl(o.x, (int)src, 64), __shfl(o.y, (int)src, 64), __shfl(o.z, (int)src, 64));
    const f3 rd = make_f3(__shfl(d.x, (int)src, 64), __shfl(d.y, (int)src, 64), __shfl(d.z, (int)src, 64));
    const float rtmin = __shfl(tmin, (int)src, 64), rtmax = __shfl(tmax, (int)src, 64);
    const float ix = slab_rcp(rd.x, slab_tiny), iy = slab_rcp(rd.y, slab_tiny), iz = slab_rcp(rd.z, slab_tiny);
    const float ox = -ro.x * ix, oy = -ro.y * iy, oz = -ro.z * iz;
    float best = rtmax;           // this helper's own nearest hit (what best_id names)
    float cull = rtmax;           // the group's nearest hit so far: a true hit distance of the same ray, culled on with <= as closest_hit culls on its own
    uint32_t best_id = kMissId;
    int node = has_ray ? s_cut[k - 2u + j] : kTraversalDone;
    uint32_t sp = 0;
    for (;;) {
        uint32_t budget = descent_cap;
        while (node >= 0) {
            const float4 n0 = nodes[node * 4 + 0];
            const float4 n1 = nodes[node * 4 + 1];
            const float4 n2 = nodes[node * 4 + 2];
            const float4 n3 = nodes[node * 4 + 3];
            const float ax = pt_fma(n0.x, ix, ox), bx = pt_fma(n0.w, ix, ox);
            const float ay = pt_fma(n0.y, iy, oy), by = pt_fma(n1.x, iy, oy);
            const float az = pt_fma(n0.z, iz, oz), bz = pt_fma(n1.y, iz, oz);
            const float lx0 = fminf(ax, bx); const float cx = pt_fma(n1.z, ix, ox);
            const float ly0 = fminf(ay, by); const float dx = pt_fma(n2.y, ix, ox);
            const float lz0 = fminf(az, bz); const float cy = pt_fma(n1.w, iy, oy);
            const float hx0 = fmaxf(ax, bx); const float dy = pt_fma(n2.z, iy, oy);
            const float hy0 = fmaxf(ay, by); const float cz = pt_fma(n2.x, iz, oz);
            const float hz0 = fmaxf(az, bz); const float dz = pt_fma(n2.w, iz, oz);
            const float tn0 = fmaxf(fmaxf(lx0, ly0), raw_maxf(lz0, rtmin));
            const float tf0 = fminf(fminf(hx0, hy0), raw_minf(hz0, cull));
            const float tn1 = fmaxf(fmaxf(fminf(cx, dx), fminf(cy, dy)), raw_maxf(fminf(cz, dz), rtmin));
            const float tf1 = fminf(fminf(fmaxf(cx, dx), fmaxf(cy, dy)), raw_minf(fmaxf(cz, dz), cull));
            const bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
            const int c0 = __builtin_bit_cast(int, n3.x), c1 = __builtin_bit_cast(int, n3.y);
            if (h0 && h1) {
                const bool swap = tn1 < tn0;
                const int near_c = swap ? c1 : c0, far_c = swap ? c0 : c1;
                stack[sp] = stack_encode<StackT>(far_c);
                sp += stride;
                node = near_c;
            } else if (h0) {
                node = c0;
            } else if (h1) {
                node = c1;
            } else if (sp == 0) {
                node = kTraversalDone;
            } else {
                sp -= stride;
                node = stack_decode(stack[sp]);
            }
            if (--budget == 0u) break;
        }
        // every lane of the wave is here: with a leaf, mid-descent (the budget ran out), or finished (it stays for the exchange below)
        if (node < 0 && node != kTraversalDone) {
            const uint32_t q = ~(uint32_t)node;
            const float4 s = sph[q];
            float t;
            if (intersect_sphere(ro, rd, rtmin, kInf, make_f3(s.x, s.y, s.z), s.w, t)) {
                const uint32_t idf = ids[q];
                if ((idf >> kIdClassShift) != kAlphaInvisible) {  // (untextured scenes: no other class needs a test, alpha_candidate<false>)
                    const uint32_t id = idf & kIdMask;
                    if (t < best || (t == best && best_id != kMissId && id < best_id)) { best = t; best_id = id; }
                }
            }
            if (sp == 0) {
                node = kTraversalDone;
            } else {
                sp -= stride;
                node = stack_decode(stack[sp]);
            }
        }
        cull = group_min(raw_minf(cull, best), k);
        if (__ballot(node != kTraversalDone) == 0ull) break;
    }
    // (best, best_id) over the group: nearer t wins, equal t -> lower id (kMissId, the largest, loses to any)
#define PT_COOP_MERGE(CTRL)                                                                                              \
    {                                                                                                                    \
        const float t2 = dpp_f32<CTRL>(best);                                                                            \
        const uint32_t id2 = dpp_u32<CTRL>(best_id);                                                                     \
        if (t2 < best || (t2 == best && id2 < best_id)) { best = t2; best_id = id2; }                                    \
    }
    PT_COOP_MERGE(kDppSwap1)
    if (k >= 4u) PT_COOP_MERGE(kDppSwap2)
    if (k >= 8u) PT_COOP_MERGE(kDppMirror8)
#undef PT_COOP_MERGE
    // back to the path's own lane: live ray number r was walked by the group of lanes starting at r * k
    const uint32_t rank = __popcll(ballot & ((1ull << lane) - 1ull));
    const int owner = (int)((rank << shift) & 63u);
    t_out = __shfl(best, owner, 64);
    id_out = __shfl(best_id, owner, 64);
}

// adds a workgroup's {node visits, sphere tests} to the lane's running totals (two atomics per workgroup)
__device__ __forceinline__ void flush_visit_counters(unsigned long long* totals, const uint32_t v[2])
{
    block_atomic_add(totals + 6, v[0]);
    block_atomic_add(totals + 7, v[1]);
}

// ------------------------------------------------------------------------------------------------ primary beams
// The pyramid of a block and its tests against boxes: pt_beam.h (compiled for the host too, for tests/test_primary_beams.py).

// One lane's work for one 8x8 block: walk the tree with the block's pyramid and write the block's record.
template <typename StackT>
__device__ __forceinline__ void beam_walk_block(const SceneView& sv, const float4* nodes, const uint32_t* ids, StackT* stack, uint32_t stride, const PixelMap& pm,
                                                const CameraParams& cam, float slack, float margin_px, uint32_t tile, uint32_t* __restrict__ lists)
{
    uint32_t* rec = lists + (size_t)tile * kBeamRecord;
    const PixelRef pr = slot_to_pixel(pm, tile << 6);  // the block's first pixel
    uint32_t count = 0;
    if (pr.valid) {
        const Beam b = make_beam(cam, pr.px, pr.py, slack, margin_px);
        if (sv.n == 1) {
            rec[1] = ids[0];
            count = 1;
        } else {
            int node = 0;
            uint32_t sp = 0;
            for (;;) {
                if (node >= 0) {
                    const float4 n0 = nodes[node * 4 + 0], n1 = nodes[node * 4 + 1], n2 = nodes[node * 4 + 2], n3 = nodes[node * 4 + 3];
                    const f3 lo0 = make_f3(n0.x, n0.y, n0.z), hi0 = make_f3(n0.w, n1.x, n1.y), lo1 = make_f3(n1.z, n1.w, n2.x), hi1 = make_f3(n2.y, n2.z, n2.w);
                    const int c0 = __builtin_bit_cast(int, n3.x), c1 = __builtin_bit_cast(int, n3.y);
                    const bool h0 = c0 >= 0 ? beam_meets_box(b, lo0, hi0) : (beam_meets_box(b, lo0, hi0) && beam_meets_leaf(b, lo0, hi0));
                    const bool h1 = c1 >= 0 ? beam_meets_box(b, lo1, hi1) : (beam_meets_box(b, lo1, hi1) && beam_meets_leaf(b, lo1, hi1));
                    if (h0 && h1) { stack[sp] = stack_encode<StackT>(c1); sp += stride; node = c0; continue; }
                    if (h0) { node = c0; continue; }
                    if (h1) { node = c1; continue; }
                } else {
                    if (count < kBeamListCap) rec[1 + count] = ids[~(uint32_t)node];
                    if (++count > kBeamListCap) break;  // overflow: the wave will traverse per ray
                }
                if (sp == 0) break;
                sp -= stride;
                node = stack_decode(stack[sp]);
            }
        }
    }
    rec[0] = count;
}

// ------------------------------------------------------------------------------------------------ reflection beams
// The first bounce off a mirror-like sphere (DESIGN.md "Reflection beams", pt_region.h): when the five rays of a block's pyramid (its four
// corners and its centre) all land on one sphere S whose material samples the specular lobe only, with a roughness of at most
// kReflMaxRoughness, the block's bounce-1 rays leave a small box around the footprint in a thin cone around the mirrored centre ray.  The
// block's region record lists every sphere whose padded leaf box meets that swept region; the primary pass serves a wave's bounce-1 rays
// from it when every active lane's spawned ray passes region_contains, and traverses otherwise.
// Fills g for the block at (px, py) from its primary-beam list (beam[1..count]: a superset of what the pyramid's rays can hit); false = no region.
__device__ __forceinline__ bool refl_region(const SceneView& sv, const CameraParams& cam, uint32_t px, uint32_t py, const uint32_t* __restrict__ beam, uint32_t count,
                                            ReflRegion& g)
{
    f3 c[4];
    beam_corners(cam, px, py, 0.0f, c);
    f3 dir[5];
    float t[5];
    for (int k = 0; k < 4; k++) dir[k] = normalize(c[k]);
    dir[4] = normalize((c[0] + c[2]) + (c[1] + c[3]));
    uint32_t s_id = kMissId;
    for (int k = 0; k < 5; k++) {
        float best = kInf;
        uint32_t best_idf = kMissId;
        for (uint32_t j = 0; j < count; j++) {
            const uint32_t idf = beam[1 + j];
            if ((idf >> kIdClassShift) == kAlphaInvisible) continue;
            const float4 s = sv.sph[idf & kIdMask];
            float tk;
            if (intersect_sphere(cam.Position, dir[k], 0.0f, kInf, make_f3(s.x, s.y, s.z), s.w, tk))
                if (tk < best || (tk == best && best_idf != kMissId && (idf & kIdMask) < (best_idf & kIdMask))) { best = tk; best_idf = idf; }
        }
        if (best_idf == kMissId || (best_idf >> kIdClassShift) != 0u) return false;  // a miss, or a sphere whose crossings an alpha test decides
        if (k > 0 && best_idf != s_id) return false;
        s_id = best_idf;
        t[k] = best;
    }
    const float4 sp = sv.sph[s_id];
    const float4 m0 = sv.mats[s_id * 4 + 0], m2 = sv.mats[s_id * 4 + 2], m3 = sv.mats[s_id * 4 + 3];
    if (sv.tex_maps && (as_uint(m3.x) & kMaterialHasMaps) != 0u) return false;  // textured: maps may change the material and the normal
    const HitFrame hc = hit_frame(cam.Position, dir[4], t[4], load3(sp), sp.w);
    // the material as hit_material forms it for a primary hit, and its lobe weights for the centre ray
    const Bsdf b = bsdf_init_pre(load3(m0), m2.x, m2.y, m2.z, m3.w, m3.z, !(m2.x < 1.0f) ? 0.0f : m2.w, hc.front);
    float w[3];
    lobe_weights(b, surf_init(hc.front, hc.N, hc.front ? hc.N : -hc.N), -dir[4], w);
    if (!(w[kLobeDiffuse] == 0.0f && w[kLobeTransmission] == 0.0f && b.Roughness <= kReflMaxRoughness)) return false;
    return region_from_hits(cam.Position, dir, t, load3(sp), sp.w, g);
}

// One lane's work for one 8x8 block after its primary-beam record (lists) is written: the block's region record.
template <typename StackT>
__device__ __forceinline__ void refl_walk_block(const SceneView& sv, const float4* nodes, const uint32_t* ids, StackT* stack, uint32_t stride, const PixelMap& pm,
                                                const CameraParams& cam, uint32_t tile, const uint32_t* __restrict__ lists, uint32_t* __restrict__ regions)
{
    uint32_t* rec = regions + (size_t)tile * kReflRecord;
    const uint32_t* beam = lists + (size_t)tile * kBeamRecord;
    const PixelRef pr = slot_to_pixel(pm, tile << 6);
    const uint32_t beam_count = beam[0];
    uint32_t count = 0;
    ReflRegion g;
    if (pr.valid && beam_count >= 1u && beam_count <= kBeamListCap && refl_region(sv, cam, pr.px, pr.py, beam, beam_count, g)) {
        region_store(g, rec);
        if (sv.n == 1) {
            rec[kReflIds] = ids[0];
            count = 1;
        } else {
            int node = 0;
            uint32_t sp = 0;
            for (;;) {
                if (node >= 0) {
                    const float4 n0 = nodes[node * 4 + 0], n1 = nodes[node * 4 + 1], n2 = nodes[node * 4 + 2], n3 = nodes[node * 4 + 3];
                    const int c0 = __builtin_bit_cast(int, n3.x), c1 = __builtin_bit_cast(int, n3.y);
                    const bool h0 = region_meets_box(g, make_f3(n0.x, n0.y, n0.z), make_f3(n0.w, n1.x, n1.y));
                    const bool h1 = region_meets_box(g, make_f3(n1.z, n1.w, n2.x), make_f3(n2.y, n2.z, n2.w));
                    if (h0 && h1) { stack[sp] = stack_encode<StackT>(c1); sp += stride; node = c0; continue; }
                    if (h0) { node = c0; continue; }
                    if (h1) { node = c1; continue; }
                } else {
                    if (count < kReflListCap) rec[kReflIds + count] = ids[~(uint32_t)node];
                    if (++count > kReflListCap) { count = 0; break; }  // overflow: no region
                }
                if (sp == 0) break;
                sp -= stride;
                node = stack_decode(stack[sp]);
            }
        }
    }
    rec[0] = count;
}

// Wave-uniform records on the scalar path.  A block's beam record, its region record and the sphere records they name belong to the whole
// wave, and no kernel writes them while a frame that reads them is in flight (pt_api.hip render_common states the rule and checks it where
// beam_cache_lookup hands the buffers out; sv.sph is written by earlier kernels of the frame's own stream only).  The kernel itself stores
// to global memory, so the compiler takes a plain load of them for a vector load (global_load -> s_waitcnt vmcnt(0), which on gfx9 also
// drains the wave's stores -> v_readfirstlane); read through the constant address space they are s_load_dword[xN]: SGPRs from the scalar
// cache, waited for with lgkmcnt.  p must be wave-uniform and aligned to V.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
template <typename V>
__device__ __forceinline__ V scalar_load(const void* p)
{
    return *(const __attribute__((address_space(4))) V*)p;
}

// The run-time test of a lane's bounce-1 ray against its block's region record: h0, h1 = the record's first sixteen words (scalar_load)
__device__ __forceinline__ bool refl_contains(u32x8 h0, u32x8 h1, f3 o, f3 d)
{
    ReflRegion g;
    g.lo = make_f3(as_float(h0[1]), as_float(h0[2]), as_float(h0[3]));
    g.hi = make_f3(as_float(h0[4]), as_float(h0[5]), as_float(h0[6]));
    g.axis = make_f3(as_float(h0[7]), as_float(h1[0]), as_float(h1[1]));
    g.cos_run = as_float(h1[2]);
    g.theta = 0.0f;
    return region_contains(g, o, d);
}

// kLds: the workgroup stages the tree into LDS first (LDS-resident scenes).  (Measured: 55 vs 58 us at 1080p -- a lane's walk is ~80 visits
// of ~150 instructions, bound by instruction issue of lone waves rather than by where the nodes live; the build stays off the frames'
// critical path: on a side stream for a resting view, behind a frame on its lane for a moving camera.  Sixteen lanes per block, each walking
// one subtree four levels down, were measured: the same 56 us beside the frames -- the build's time is its share of a busy chip, not its chain.)
// regions (resting views; null = none): the blocks' reflection-beam records, made after their primary-beam records.
template <bool kLds, typename StackT>
__global__ __launch_bounds__(256) void beam_kernel(SceneView sv, PixelMap pm, FrameParams fp, float slack, uint32_t* __restrict__ lists, uint32_t* __restrict__ regions)
{
    const uint32_t stride = blockDim.x;
    const uint32_t n_blocks = pm.n_slots >> 6;
    TreeWalk<StackT> tw;
    tree_walk_setup<kLds, StackT>(sv, tw);
    const auto [nodes, sph, ids, stack] = tw;  // (the beams read no sphere record: sph is unused)
    for (uint32_t tile = blockIdx.x * blockDim.x + threadIdx.x; tile < n_blocks; tile += gridDim.x * blockDim.x)
    {
        beam_walk_block<StackT>(sv, nodes, ids, stack, stride, pm, fp.cam, slack, 0.0f, tile, lists);
        if (regions) refl_walk_block<StackT>(sv, nodes, ids, stack, stride, pm, fp.cam, tile, lists, regions);
    }
}

// A candidate list as its reader holds it: where the ids stand in the record, how many there are (walked when 1 .. cap), the first three of them
// (they come with the record's first words: one scalar round trip) and the first one's sphere record (a second, begun as soon as the
// first is back and long before the list is walked).  All wave-uniform.
struct ListHead {
    const uint32_t* ids;
    uint32_t count, cap;
    uint32_t id0, id1, id2;
    u32x4 s0;
};

// the first candidate's sphere (the ids carry their alpha class); a list with no entry names none
__device__ __forceinline__ u32x4 list_first_sphere(const SceneView& sv, uint32_t count, uint32_t cap, uint32_t id0)
{
    u32x4 s0 = { 0u, 0u, 0u, 0u };
    if (count - 1u < cap) s0 = scalar_load<u32x4>(sv.sph + (id0 & kIdMask));
    return s0;
}

// Closest hit of a ray over its block's candidate list (wave-uniform loop).  Same candidates, same order, same intersect_sphere, same
// tie rule as closest_hit's leaves.  Nothing the loop reads comes through the vector memory path: while candidate j is intersected, the
// sphere of candidate j + 1 and the id of candidate j + 3 are under way as scalar loads (the ids two entries ahead of the spheres, since
// a sphere's address needs its id), so an iteration waits for neither.  The loads ahead stay inside the record (the id index is clamped
// to the record's last word) and inside sv.sph (past the list's end the current candidate's sphere is fetched again).
template <bool kAlphaTex = false>
__device__ __forceinline__ void closest_hit_list(const SceneView& sv, const ListHead& L, f3 o, f3 d, float tmin, float tmax, float& t_out, uint32_t& id_out)
{
    float best = tmax;
    uint32_t best_id = kMissId;
    uint32_t idf = L.id0, idf1 = L.id1, idf2 = L.id2;  // (the list carries the leaf ids with their alpha class)
    u32x4 sb = L.s0;
    // (scalar loads return in any order, so a wait for one is a wait for all: L.s0 is waited for here, where nothing else is under way -- left
    // to the loop's first use it would be a wait behind the loads ahead in every iteration.  gfx9 encoding: lgkmcnt(0), vmcnt and expcnt open.)
    __builtin_amdgcn_s_waitcnt(0xC07F);
    for (uint32_t j = 0; j < L.count; j++) {
        const u32x4 sb1 = scalar_load<u32x4>(sv.sph + ((j + 1u < L.count ? idf1 : idf) & kIdMask));
        const uint32_t idf3 = scalar_load<uint32_t>(L.ids + (j + 3u < L.cap ? j + 3u : L.cap - 1u));
        if ((idf >> kIdClassShift) != kAlphaInvisible) {  // wave-uniform
            const uint32_t id = idf & kIdMask;
            const float4 s = make_float4(as_float(sb.x), as_float(sb.y), as_float(sb.z), as_float(sb.w));
            float t;
            if (intersect_sphere(o, d, tmin, kInf, make_f3(s.x, s.y, s.z), s.w, t)) {
                if ((idf >> kIdClassShift) == 0u || alpha_candidate<kAlphaTex>(sv, idf, make_f3(s.x, s.y, s.z), s.w, o, d, t))
                    if (t < best || (t == best && best_id != kMissId && id < best_id)) { best = t; best_id = id; }
            }
        }
        idf = idf1; idf1 = idf2; idf2 = idf3; sb = sb1;
    }
    t_out = best; id_out = best_id;
}

// ------------------------------------------------------------------------------------------------ shade
// Per-path state carried between kernels in the ray queue (48 B) -- see RayQueue in pt_device.h.
struct PathState {
    f3 o, d, T;
    uint32_t slot, rng, bounce, sample;
    bool dirty;  // scratch.sample_rad[slot] holds this sample's radiance so far
    bool via_t;  // the sample left the primary surface through the transmission lobe (direct illumination does not cover it)
    bool dn_spec;  // denoiser frames (kDn): sample 0 left the primary surface through a lobe other than diffuse (kFlagDnSpecular)
};

// One iteration of the bounce-loop body (Raytracing.hlsl:213-364) for a path whose ray (ps.o, ps.d) has been traced to
// (t, id); on sample end it accumulates into the pixel, and either finishes the pixel or regenerates the next sample
// from the cached primary hit and keeps going.  Returns true when ps holds a new ray that must be traced.
// the material of a hit (pt_surface.h; HitMaterial: frame, EvaluateMaterial, BSDFSample)
template <bool kTex>
__device__ __forceinline__ HitMaterial hit_material(const SceneView& sv, uint32_t id, f3 o, f3 d, float t, bool primary)
{
    return hit_material_at<kTex>(sv.sph, sv.mats, sv.tex, sv.tex_maps, sv.rot, id, o, d, t, primary);
}

// kMulti = false specialises for SamplesPerPixel == 1: no radiance accumulator, no primary-hit cache, no sample
// regeneration (and with it no camera parameters live across the bounce loop).
// kTex = true adds EvaluateMaterial's texture branches + normal mapping (row N1; csrc/pt_texture.h).  It is a template
// parameter of every kernel that shades, chosen per launch from SceneView::tex_maps, so the kernels of the untextured hot
// path carry none of it (the textured fused kernels need 122-128 VGPRs against 101-107).
// Row N4: the direct-illumination estimate of a primary surface (csrc/pt_light.h; oracle render_pixel): ONE emissive sphere chosen
// uniformly, a direction uniformly inside the cone it subtends, a shadow ray through `trace` (the ordinary closest-hit query:
// the emitter must be the first thing it meets), DI = Le * (f_diffuse + f_specular) cos * n_lights / pdf with Le evaluated at the
// point the shadow ray reaches (EvaluateMaterial: an emissive map modulates it).  Own per-pixel RNG stream.
// kSplit (row N7, the NRD modes of denoiser frames): also the estimate's diffuse and specular halves, (Le * f_d) * k and (Le * f_s) * k,
// zeroed wherever the sum is (halves[0], halves[1]); the sum is formed exactly as without the split.
template <bool kTex, bool kSplit = false, typename TraceFn>
__device__ __forceinline__ f3 di_estimate(const SceneView& sv, const FrameParams& fp, uint32_t px, uint32_t py, uint32_t id, f3 d, const HitMaterial& hm,
                                          TraceFn&& trace, uint32_t& rays, f3* halves = nullptr)
{
    f3 est = make_f3(0.f, 0.f, 0.f);
    f3 est_d = est, est_s = est;  // kSplit only
    uint32_t rng = rng_init(px, py, fp.frame_index ^ kDiRngSalt);
    const float u0 = rng_float(rng), u1 = rng_float(rng), u2 = rng_float(rng);
    const uint32_t light = sv.lights[pick_light(u0, sv.n_lights)];
    const float4 ls = sv.sph[light];
    const LightSample s = sample_sphere_cone(hm.hf.P, load3(ls), ls.w, u1, u2);
    const Surf surf = surf_init(hm.hf.front, hm.hf.N, hm.Ns);
    if (light != id && s.valid && dot(surf.FrontNg, s.L) > 0.0f) {
        const f3 V = -d;
        float w[3];
        lobe_weights(hm.bsdf, surf, V, w);
        f3 f, f_d, f_s;
        if (kSplit) { bsdf_eval_reflective_lobes(hm.bsdf, surf, s.L, V, w, f_d, f_s); f = f_d + f_s; }
        else f = bsdf_eval_reflective(hm.bsdf, surf, s.L, V, w);
        // No shadow ray for a contribution that cannot matter: the estimate's upper bound with the emitter's untextured radiance
        // (maps modulate it downwards) is below kDiNegligible -- a mirror-like primary surface seen off its specular direction,
        // i.e. most of the demo's ground.  (Bias below 1e-7 of unit radiance per pixel; spec of this row, not of the reference.)
        const float4 lm = sv.mats[light * 4 + 1];  // {EmissiveStrength, EmissiveColor}
        const float k = s.inv_pdf * (float)sv.n_lights;
        const float bound = pt_max(f.x * lm.y, pt_max(f.y * lm.z, f.z * lm.w)) * (lm.x * k);
        if (bound > kDiNegligible) {
            float t2;
            uint32_t id2;
            const f3 so = spawn_origin(hm.hf.P, hm.hf.N, hm.hf.offset, s.L);
            trace(so, s.L, t2, id2);
            rays++;
            if (id2 == light) {
                const f3 le = hit_material<kTex>(sv, light, so, s.L, t2, false).emission;
                est = (le * f) * k;
                if (kSplit) { est_d = (le * f_d) * k; est_s = (le * f_s) * k; }
            }
        }
    }
    if (!(est.x > 0.0f || est.y > 0.0f || est.z > 0.0f) || !is_finite(est.x) || !is_finite(est.y) || !is_finite(est.z)) {
        est = make_f3(0.f, 0.f, 0.f);  // NaN / inf / negative estimates count as no light
        est_d = est; est_s = est;
    }
    if (kSplit) { halves[0] = est_d; halves[1] = est_s; }
    return est;
}

struct NoTrace {
    __device__ __forceinline__ void operator()(f3, f3, float&, uint32_t&) const {}
};

// kDI = true (primary passes of the fused schedule): the direct-illumination estimate is made HERE, at the first shading of the
// primary surface, sharing its material / BSDF evaluation; `trace` casts the shadow ray, `di_rays` counts it.  With kDI = false
// and fp.di_enabled the estimate is read from scratch.di (written by a kDI pass or, in the split schedule, by di_kernel).
// kCacheMode (kMulti, untextured kernels; Scratch::primary_cache): 1 = the primary pass stores what the first shading of the primary
// surface computed (plus where the pixel is written); 2 = the looping pass restarts a pixel's next sample from that record instead of recomputing the primary ray, the
// hit frame and the lobe weights (~250 of the ~1100 instructions of a full shading step, once per sample: all samples of a pixel share
// their primary hit, Raytracing.hlsl:193-198).  The cached values are the ones the full path computes, bit for bit.
// kMerge (the looping pass at spp > 1): ONE pass through the surface-shading code per call.  The plain form shades the traced hit,
// and when that ends the sample loops back to shade the regenerated primary hit -- two passes through the most expensive code of the
// kernel, each for a fraction of the wave's lanes (92 % of C3's bounce rays miss: the first pass runs for the few lanes that hit).
// Merged, a lane whose ray missed finishes its sample first and then shades its regenerated primary hit TOGETHER with the lanes that
// hit; a lane whose sample ends in the surface code returns kShadePending and starts its next call there (no ray to trace in between).
// Per-lane order of operations, RNG draws and arithmetic are unchanged.  `pending` in: the previous call returned kShadePending.
// kDn (row N7, DESIGN.md spec S13; frames of pt_render_denoiser, scratch.dn.mode != 0): the pixel's finish writes the denoiser outputs.  The
// first shading of sample 0's primary surface leaves {prim, hd = +inf} in scratch.dn.rec, sample 0's lobe at bounce 0 rides in the path's
// flags (ps.dn_spec), its bounce-1 hit replaces hd; with kDI the estimate goes straight to scratch (split by lobe in the NRD modes).
enum : int { kShadeDone = 0, kShadeRay = 1, kShadePending = 2 };

// kBlock (the 1-spp primary pass): the wave's slots are one 8x8 block and `bo` is its origin, made once per tile on the scalar unit
// (block_origin): a pixel write forms its index from it in three instructions, and nothing here maps the slot again.
template <bool kMulti, bool kTex = false, bool kDI = false, int kCacheMode = 0, bool kMerge = false, bool kDn = false, bool kBlock = false, typename TraceFn = NoTrace>
__device__ __forceinline__ int shade_step_ex(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const Scratch& scratch,
                                             float4* __restrict__ out, PathState& ps, float t, uint32_t id, bool pending, TraceFn&& trace = NoTrace(), uint32_t* di_rays = nullptr,
                                             const BlockOrigin* bo = nullptr)
{
    static_assert(!kMerge || (kMulti && !kDI), "the merged form is the looping pass of spp > 1 frames");
    static_assert(!kBlock || !kMulti, "the block form is the 1-spp primary pass");
    const uint32_t slot = ps.slot;
    auto pixel_of_slot = [&]() -> PixelRef { return kBlock ? block_pixel(*bo, slot & 63u) : slot_to_pixel(pm, slot); };
    auto out_index_of_slot = [&]() -> uint32_t { return kBlock ? block_out_index(*bo, slot & 63u) : slot_to_pixel(pm, slot).out_index; };
    f3 di_val = make_f3(0.f, 0.f, 0.f);
    bool di_have = false;  // di_val is this pixel's estimate, made in this call
    bool regen = false;    // kCacheMode 2: the surface being shaded is a regenerated primary hit described by the pixel's cached record
    float4 rc0 = make_float4(0.f, 0.f, 0.f, 0.f), rc1 = rc0;
    // sampleRadiance so far is (dirty ? scratch : 0); srad_loaded says whether `srad` holds it
    f3 srad = make_f3(0.f, 0.f, 0.f);
    bool srad_loaded = false, srad_changed = false;
    bool end_sample = false;
    f3 L = make_f3(0.f, 0.f, 0.f);
    HitFrame hf;

    // the ray missed: sampleRadiance += T * environment (:242-259); a primary miss writes the pixel and returns true
    auto shade_miss = [&]() -> bool {
        f3 env;
        if (kTex && sv.env_tex != kNoTexture)
            env = sv.env_cube ? environment_cube(sv.tex + sv.env_tex, sv.env_xf, ps.d) : environment_texture(sv.tex[sv.env_tex], sv.env_xf, ps.d);
        else env = environment_color(sv.env[0], sv.env[1], sv.env[2], sv.env[3], ps.d);
        if (!kMerge && ps.bounce == 0) {  // primary miss: pixel = environment (GBufferGeneration.hlsl:223-227; Raytracing.hlsl:249-252); the looping pass only sees paths with a primary hit
            out[out_index_of_slot()] = make_float4(env.x, env.y, env.z, 1.0f);
            return true;
        }
        if (ps.dirty) { const float4 s = scratch.sample_rad[slot]; srad = load3(s); }
        srad_loaded = true;
        srad = srad + ps.T * env;  // :254
        end_sample = true;
        return false;
    };

    // the ray hit sphere `id` at t (or: the regenerated primary hit): material, emission, lobe choice, sample, pdf, f, throughput,
    // Russian roulette, cut-off (:293-364).  Sets end_sample, or leaves L / hf for the spawn.
    auto shade_surface = [&]() {
        HitMaterial hm;
        if (kCacheMode == 2 && regen) {
            // the primary hit of this pixel again: frame and weights from the record (rc0 = {N, offset}, rc1 = {weights, id}), the
            // material as hit_material forms it (bounce 0: Transmission = Metallic < 1 ? Transmission : 0, Raytracing.hlsl:148)
            const float4 sp = sv.sph[id];
            const float4 m0 = sv.mats[id * 4 + 0], m1 = sv.mats[id * 4 + 1], m2 = sv.mats[id * 4 + 2], m3 = sv.mats[id * 4 + 3];
            hm.hf.N = make_f3(rc0.x, rc0.y, rc0.z);
            hm.hf.P = mad(sp.w, hm.hf.N, load3(sp));
            hm.hf.offset = rc0.w;
            hm.hf.front = dot(hm.hf.N, ps.d) < 0.0f;
            hm.Ns = hm.hf.front ? hm.hf.N : -hm.hf.N;
            hm.emission = make_f3(m1.y, m1.z, m1.w) * m1.x;
            hm.bsdf = bsdf_init_pre(load3(m0), m2.x, m2.y, m2.z, m3.w, m3.z, !(m2.x < 1.0f) ? 0.0f : m2.w, hm.hf.front);
        } else {
            hm = hit_material<kTex>(sv, id, ps.o, ps.d, t, ps.bounce == 0);
        }
        hf = hm.hf;
        if (kDn && (!kMulti || ps.sample == 0)) {
            if (ps.bounce == 0) scratch.dn.rec[slot] = make_float4(hm.emission.x, hm.emission.y, hm.emission.z, kInf);  // prim (= G-buffer Radiance), hd default
            else if (ps.bounce == 1) reinterpret_cast<float*>(scratch.dn.rec + slot)[3] = t;  // sample 0's bounce-1 ray hit at t (a miss keeps +inf)
        }
        f3 emission = hm.emission;
        const f3 Ns = hm.Ns;
        const Bsdf& bsdf = hm.bsdf;
        // Sphere-light direct illumination (row N4) covers what the reflective lobes of the primary surface receive from the
        // emitters, so the emission of a first-bounce hit reached through them is dropped (Raytracing.hlsl:302).  The flag
        // is "the pixel has a primary surface", not the reference's any(DI > 0): with a one-sample estimator DI = 0 is an
        // ordinary sample value and conditioning on it would bias the frame upward; and a sample that left through the
        // transmission lobe keeps its emission, because DI evaluates the reflective lobes only.
        if (fp.di_enabled && ps.bounce == 1 && !ps.via_t) emission = make_f3(0.f, 0.f, 0.f);
        if (kDI && fp.di_enabled && ps.bounce == 0 && (!kMulti || ps.sample == 0) && !di_have) {
            const PixelRef dpr = pixel_of_slot();
            if (kDn) {  // stored at once (the finish reads it back): no estimate lives across the bounce in registers
                f3 halves[2];
                const f3 est = di_estimate<kTex, true>(sv, fp, dpr.px, dpr.py, id, ps.d, hm, trace, *di_rays, halves);
                if (scratch.dn.mode == 1) {
                    scratch.di[slot] = make_float4(est.x, est.y, est.z, 0.f);
                } else {
                    scratch.di[slot] = make_float4(halves[0].x, halves[0].y, halves[0].z, 0.f);
                    scratch.dn.di_s[slot] = make_float4(halves[1].x, halves[1].y, halves[1].z, 0.f);
                }
            } else {
                di_val = di_estimate<kTex>(sv, fp, dpr.px, dpr.py, id, ps.d, hm, trace, *di_rays);
                di_have = true;
            }
        }
        const bool t_finite = is_finite(ps.T.x) && is_finite(ps.T.y) && is_finite(ps.T.z);
        if (emission.x != 0.0f || emission.y != 0.0f || emission.z != 0.0f || !t_finite) {
            if (ps.dirty) { const float4 s = scratch.sample_rad[slot]; srad = load3(s); }
            srad_loaded = true;
            srad = srad + ps.T * emission;  // :320
            srad_changed = true;
        }
        const bool last = ps.bounce == fp.bounces;
        if (last && (!kMulti || ps.sample + 1 == fp.spp)) {
            end_sample = true;  // the sample drawn on the final iteration is never used and no later sample reads the RNG
            return;
        }
        // Ns is hit_material's: +-hit_frame's normal or perturb_normal's result, both outputs of normalize() (the regenerated hit reads back the
        // normal that this code stored), which is what get_basis_unit's range proof needs
        const Surf surf = surf_init_unit(hf.front, hf.N, Ns);
        const f3 V = -ps.d;
        float w[3];
        if (kCacheMode == 2 && regen) {
            w[0] = rc1.x; w[1] = rc1.y; w[2] = rc1.z;
        } else {
            lobe_weights(bsdf, surf, V, w);
            if (kCacheMode == 1 && scratch.primary_cache && ps.bounce == 0 && ps.sample == 0) {
                float4* rec = scratch.primary_cache + (size_t)slot * 3u;
                rec[0] = make_float4(hf.N.x, hf.N.y, hf.N.z, hf.offset);
                rec[1] = make_float4(w[0], w[1], w[2], as_float(id));
                rec[2] = make_float4(ps.d.x, ps.d.y, ps.d.z, as_float(out_index_of_slot()));  // (where the pixel is written: the looping pass needs no slot -> pixel mapping)
            }
        }
        float rnd[4];
        rnd[0] = rng_float(ps.rng); rnd[1] = rng_float(ps.rng); rnd[2] = rng_float(ps.rng); rnd[3] = rng_float(ps.rng);  // :330
        int lobe;
        if (!bsdf_sample(bsdf, surf, V, w, rnd, L, lobe)) { end_sample = true; return; }
        float pdf;
        f3 f;
        if (!bsdf_pdf_eval(bsdf, surf, L, V, w, lobe, pdf, f)) { end_sample = true; return; }  // pdf == 0 (:336-339)
        if (f.x == 0.0f && f.y == 0.0f && f.z == 0.0f) { end_sample = true; return; }
        { const float inv_pdf = pt_rcp(pdf); ps.T = ps.T * (f * inv_pdf); }  // :346
        if (ps.bounce == 0) ps.via_t = lobe == kLobeTransmission;
        if (fp.rr_enabled && ps.bounce > 3) {                     // :348-356
            const float p = pt_max(ps.T.x, pt_max(ps.T.y, ps.T.z));
            if (rng_float(ps.rng) >= p) end_sample = true;
            else ps.T = ps.T * pt_rcp(p);
        }
        if (!end_sample && luminance(ps.T) <= fp.throughput_threshold) end_sample = true;  // :361
        if (last) end_sample = true;
        if (kDn && !end_sample && ps.bounce == 0 && (!kMulti || ps.sample == 0)) ps.dn_spec = lobe != kLobeDiffuse;  // (transmission counts as specular)
    };

    // spawn the next ray (Raytracing.hlsl:219-224)
    auto spawn = [&]() {
        ps.o = spawn_origin(hf.P, hf.N, hf.offset, L);
        ps.d = L;
        ps.bounce++;
        if (srad_changed) { scratch.sample_rad[slot] = make_float4(srad.x, srad.y, srad.z, 0.f); ps.dirty = true; }
        if (kDI && di_have) scratch.di[slot] = make_float4(di_val.x, di_val.y, di_val.z, 0.f);  // the pass that finishes the pixel adds it
    };

    // end of sample: radiance += sampleRadiance (:373); true = that was the pixel's last sample, the pixel has been written (:378-385)
    auto finish_sample = [&]() -> bool {
        if (!srad_loaded) {
            if (ps.dirty) { const float4 s = scratch.sample_rad[slot]; srad = load3(s); }
        }
        f3 acc = make_f3(0.f, 0.f, 0.f);
        if (kMulti && ps.sample > 0) { const float4 r = scratch.radiance[slot]; acc = load3(r); }
        const f3 total = acc + srad;
        ps.sample++;
        if (!kMulti || ps.sample == fp.spp) {
            f3 res = make_f3(0.f, 0.f, 0.f);
            if (is_finite(total.x) && is_finite(total.y) && is_finite(total.z)) {
                res = total * fp.inv_spp;
            }
            if (kDn) {  // spec S13, by mode (Raytracing.hlsl:377-414)
                const uint32_t out_index = kCacheMode == 2 ? as_uint(scratch.primary_cache[(size_t)slot * 3u + 2u].w) : out_index_of_slot();
                const float4 rec = scratch.dn.rec[slot];
                const bool diffuse = !ps.dn_spec;
                if (scratch.dn.mode == 1) {  // DLSS-RR: the radiance of pt_render, and the hit distance of a specular first bounce
                    if (fp.di_enabled) { const float4 di = scratch.di[slot]; res = res + load3(di); }
                    out[out_index] = make_float4(res.x, res.y, res.z, 1.0f);
                    if (!diffuse && is_finite(rec.w)) scratch.dn.spec_hit_dist[out_index] = rec.w;
                } else {  // NRD: the primary emission; the rest by the lobe of the first bounce, with the DI halves
                    const f3 prim = load3(rec);
                    const f3 ind = make_f3(pt_max(res.x - prim.x, 0.0f), pt_max(res.y - prim.y, 0.0f), pt_max(res.z - prim.z, 0.0f));
                    f3 di_d = make_f3(0.f, 0.f, 0.f), di_s = di_d;
                    if (fp.di_enabled) { const float4 a = scratch.di[slot], b = scratch.dn.di_s[slot]; di_d = load3(a); di_s = load3(b); }
                    const f3 zero = make_f3(0.f, 0.f, 0.f);
                    const f3 dif = di_d + (diffuse ? ind : zero), spe = di_s + (diffuse ? zero : ind);
                    scratch.dn.diffuse[out_index] = make_float4(dif.x, dif.y, dif.z, diffuse ? rec.w : 0.0f);
                    scratch.dn.specular[out_index] = make_float4(spe.x, spe.y, spe.z, diffuse ? 0.0f : rec.w);
                    out[out_index] = make_float4(prim.x, prim.y, prim.z, 1.0f);
                }
                return true;
            }
            if (fp.di_enabled) {  // radiance += DI (:381)
                if (kDI && di_have) res = res + di_val;
                else { const float4 di = scratch.di[slot]; res = res + load3(di); }
            }
            const uint32_t out_index = kCacheMode == 2 ? as_uint(scratch.primary_cache[(size_t)slot * 3u + 2u].w) : out_index_of_slot();
            out[out_index] = make_float4(res.x, res.y, res.z, 1.0f);
            return true;
        }
        scratch.radiance[slot] = make_float4(total.x, total.y, total.z, 0.f);
        return false;
    };

    // regenerate: every sample restarts from the same primary ray / primary hit (:193-198)
    auto regenerate = [&]() {
        if (kCacheMode == 2) {  // (the host hands kernels of this mode the records: render_common)
            const float4* rec = scratch.primary_cache + (size_t)slot * 3u;
            rc0 = rec[0]; rc1 = rec[1];
            const float4 rc2 = rec[2];
            ps.o = fp.cam.Position;
            ps.d = make_f3(rc2.x, rc2.y, rc2.z);
            id = as_uint(rc1.w);
            regen = true;
        } else {
            const PixelRef pr = slot_to_pixel(pm, slot);
            float tmin, tmax;
            primary_ray(fp.cam, pr.px, pr.py, ps.o, ps.d, tmin, tmax);
            const uint2 ph = scratch.primary_hit[slot];
            t = as_float(ph.x);
            id = ph.y;
        }
        ps.T = make_f3(1.f, 1.f, 1.f);
        ps.bounce = 0;
        ps.dirty = false;
        ps.via_t = false;
        srad = make_f3(0.f, 0.f, 0.f);
        srad_loaded = false; srad_changed = false;
        end_sample = false;
    };

    if (kMerge) {
        if (pending) {
            regenerate();
        } else if (id == kMissId) {
            if (shade_miss()) return kShadeDone;
            if (finish_sample()) return kShadeDone;
            regenerate();
        }
        shade_surface();  // the traced hit, or the regenerated primary hit of a lane whose ray missed / whose last call ended its sample
        if (!end_sample) { spawn(); return kShadeRay; }
        return finish_sample() ? kShadeDone : kShadePending;
    }
    for (;;) {
        if (id == kMissId) { if (shade_miss()) return kShadeDone; }
        else shade_surface();
        if (!end_sample) { spawn(); return kShadeRay; }
        if (finish_sample()) return kShadeDone;
        regenerate();
    }
}

// One iteration of the bounce-loop body for a path whose ray (ps.o, ps.d) has been traced to (t, id), as the kernels outside the merged
// looping pass use it: true = ps holds a new ray that must be traced, false = the pixel is finished.
template <bool kMulti, bool kTex = false, bool kDI = false, int kCacheMode = 0, bool kDn = false, bool kBlock = false, typename TraceFn = NoTrace>
__device__ __forceinline__ bool shade_step(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const Scratch& scratch,
                                           float4* __restrict__ out, PathState& ps, float t, uint32_t id, TraceFn&& trace = NoTrace(), uint32_t* di_rays = nullptr,
                                           const BlockOrigin* bo = nullptr)
{
    return shade_step_ex<kMulti, kTex, kDI, kCacheMode, false, kDn, kBlock>(sv, pm, fp, scratch, out, ps, t, id, false, trace, di_rays, bo) == kShadeRay;
}

// kDn: the queue record also carries PathState::dn_spec (kFlagDnSpecular; denoiser frames)
template <bool kDn = false>
__device__ __forceinline__ PathState load_path(const RayQueue& q, uint32_t i)
{
    const float4 a = q.q0[i], b = q.q1[i], c = q.q2[i];
    PathState ps;
    ps.o = load3(a); ps.d = load3(b); ps.T = load3(c);
    ps.slot = as_uint(a.w); ps.rng = as_uint(b.w);
    const uint32_t flags = as_uint(c.w);
    ps.bounce = flags & kFlagBounceMask;
    ps.sample = (flags >> kFlagSampleShift) & kFlagSampleMask;
    ps.dirty = (flags & kFlagDirty) != 0;
    ps.via_t = (flags & kFlagViaTransmission) != 0;
    ps.dn_spec = kDn && (flags & kFlagDnSpecular) != 0;
    return ps;
}

template <bool kDn = false>
__device__ __forceinline__ void store_path(const RayQueue& q, uint32_t j, const PathState& ps)
{
    const uint32_t flags = (ps.bounce & kFlagBounceMask) | ((ps.sample & kFlagSampleMask) << kFlagSampleShift) | (ps.dirty ? kFlagDirty : 0u)
                           | (ps.via_t ? kFlagViaTransmission : 0u) | (kDn && ps.dn_spec ? kFlagDnSpecular : 0u);
    q.q0[j] = make_float4(ps.o.x, ps.o.y, ps.o.z, as_float(ps.slot));
    q.q1[j] = make_float4(ps.d.x, ps.d.y, ps.d.z, as_float(ps.rng));
    q.q2[j] = make_float4(ps.T.x, ps.T.y, ps.T.z, as_float(flags));
}

// Cold kernel arguments.  A by-value kernel argument is loaded into SGPRs at the kernel's entry and stays there: with ~120 dwords of
// arguments and 100 SGPRs, the camera and the pixel map -- needed once per batch, to generate the primary rays -- lived in VGPR lanes
// and came back through ~70 v_readlane per batch (VALU issue slots, in a VALU-bound kernel).  cold_arg re-reads such an argument from the
// kernarg segment where it is used (s_load, scalar cache): the laundered pointer keeps the loads inside the loop.
// The leading arguments of bounce_kernel, as the kernarg segment lays them out (in order, each at its natural alignment = a C struct):
struct BounceArgHead { SceneView sv; PixelMap pm; FrameParams fp; };
struct BounceArgs { SceneView sv; PixelMap pm; FrameParams fp; RayQueue qin, qout; Scratch scratch; float4* out; const uint32_t* count_in; uint32_t* count_out; FrameCounters fc; };  // ... and all of them
template <typename T>
__device__ __forceinline__ T cold_arg(uint32_t offset)
{
    // (read word by word through a dword pointer: the laundering hides the segment's alignment with its origin, and a load the compiler
    // takes for byte-aligned cannot be a scalar one -- it became global_load -> s_waitcnt vmcnt -> v_readfirstlane, once per tile)
    static_assert(sizeof(T) % 4u == 0u && alignof(T) >= 4u, "cold_arg: whole dwords");
    const __attribute__((address_space(4))) char* p = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    const __attribute__((address_space(4))) uint32_t* q = (const __attribute__((address_space(4))) uint32_t*)(p + offset);
    uint32_t w[sizeof(T) / 4u];
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T) / 4u; k++) w[k] = q[k];
    T v;
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

// The trace -> shade loop of a wave of 1-spp paths with the cooperative walk: the wave meets at every trace, and a lane whose path has ended
// (or that never had one) stays as a helper until no lane of the wave holds a live path.  Every path keeps its own state, RNG stream and shading;
// only who performs which slab and sphere tests changes.  More than 32 live paths leave no helpers: the per-lane walk.  `rays` counts the rays
// spawned here.
template <typename StackT, bool kDn>
__device__ __forceinline__ void coop_bounces(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const Scratch& scratch, float4* __restrict__ out,
                                             const float4* __restrict__ nodes, const float4* __restrict__ sph, const uint32_t* __restrict__ ids,
                                             const int* __restrict__ s_cut, StackT* stack, uint32_t stride, PathState& ps, bool alive, uint32_t& rays)
{
    for (;;) {
        const unsigned long long ballot = __ballot(alive);
        if (ballot == 0ull) break;
        float t = 0.0f;
        uint32_t id = kMissId;
        if (__popcll(ballot) > 32) {
            if (alive) closest_hit<StackT, false, false, false>(sv, nodes, sph, ids, sv.n, ps.o, ps.d, 0.0f, kInf, stack, stride, t, id, nullptr, sv.descent_cap);
        } else {
            closest_hit_coop<StackT>(nodes, sph, ids, s_cut, ballot, ps.o, ps.d, 0.0f, kInf, stack, stride, t, id, sv.descent_cap, sv.slab_tiny);
        }
        if (alive) {
            alive = shade_step<false, false, false, 0, kDn>(sv, pm, fp, scratch, out, ps, t, id);
            if (alive) rays++;
        }
    }
}

// ------------------------------------------------------------------------------------------------ fused bounce
// trace + shade in one kernel (DESIGN.md "Kernels"): a lane obtains a ray (kPrimary: generated from its pixel; else read
// from the input queue), traces it, and runs one shade_step.  kLoop = false: survivors are compacted into the output
// queue (wave64 ballot + prefix, one atomic per workgroup) -- one wavefront bounce per launch, 96 B of queue traffic
// per ray and no hit stream.  kLoop = true: the lane keeps alternating trace and shade_step until its pixel is done
// (the persistent "tail" form for small queues).  kDn: the instance of a denoiser frame (shade_step_ex; row N7).
template <bool kLds, typename StackT, bool kPrimary, bool kLoop, bool kMulti, bool kTex, bool kInline2, bool kFuse, bool kDI, bool kDn>
// 4 waves/SIMD (<= 128 VGPRs): two 512-thread workgroups per CU with the BVH in LDS (the unconstrained build takes 134
// VGPRs for the primary variant and drops to 3 waves/SIMD: measured 171 -> 149 us for the two compacting passes at C2)
__global__ __launch_bounds__(kFusedThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void bounce_kernel(SceneView sv, PixelMap pm, FrameParams fp, RayQueue qin, RayQueue qout,
                                                               Scratch scratch, float4* __restrict__ out,
                                                               const uint32_t* __restrict__ count_in_ptr, uint32_t* __restrict__ count_out_ptr,
                                                               FrameCounters fc)
{
    // Bounces traced per lane before the survivors are compacted.  The primary pass of a 1-spp frame takes TWO (the primary
    // ray and, in registers, the first bounce ray of the ~49 % of pixels that hit something): the ~1.0 M bounce-1 rays of a
    // 1080p frame then never travel through HBM (96 MB per frame) and the most latency-exposed pass of the frame (a
    // separate queue-fed bounce-1 launch, 63 % of its wave time in s_waitcnt) disappears; the half-empty waves cost less
    // than that.  Measured on C2: 1 bounce 0.1165, 2 bounces 0.107, 3 bounces 0.116, 4 bounces 0.123 ms per frame (kInline2 is
    // the host's switch; it is on for every 1-spp frame of the fused schedule).
    constexpr uint32_t kIters = (kPrimary && !kLoop && !kMulti && kInline2) ? 2u : 1u;
    // The looping pass of a 1-spp frame is a chain of dependent bounces on a few thousand nearly empty waves that share their SIMDs with the
    // primary passes of the frames behind it.  VALU issue is arbitrated by priority, then age (MI355X_MICROARCH.md), and those primary waves are
    // usually the older ones: raised priority lets the chain run as if alone, for a handful of issue slots taken from the throughput-bound waves.
    if (kLoop && !kMulti && !kPrimary) __builtin_amdgcn_s_setprio(3);
    extern __shared__ float4 smem[];
    __shared__ uint32_t s_wave_count[kFusedThreads / 64];
    __shared__ uint32_t s_block_base;
    __shared__ uint32_t s_seg_count;                  // producer side of the segmented hand-over (FrameCounters::seg_counts)
    __shared__ uint32_t s_seg_next;                   // ... and the next 64-slot tile of this workgroup's batches to hand to a wave
    __shared__ uint32_t s_loop_next;                  // fused form: the next 64 entries of the workgroup's own segment
    __shared__ uint32_t s_seg_prefix[kMaxSegs + 1];   // consumer side: s_seg_prefix[b] = entries in segments < b
    __shared__ uint32_t s_refl[2];                    // kIters == 2: waves that traced bounce-1 rays, ... of them served by a region list
    __shared__ int s_cut[kCutSlots];                  // kCoop: the tree's cuts at depths 1-3 (build_cut)
    __shared__ uint16_t s_tile_order[kTileTable];     // seg_out over beam lists: the workgroup's tiles in the order its waves draw them (below)
    __shared__ uint32_t s_tile_n;                     // ... and how many the table holds (0: none, the slot order)
    // The cooperative walk (closest_hit_coop): the looping pass of a 1-spp frame over an untextured LDS-resident scene, and the fused form's tail
    constexpr bool kCoop = kLds && !kMulti && !kTex && !kDI && !kDn && sizeof(StackT) == 2 && ((kLoop && !kPrimary) || kFuse);
    if (kPrimary && blockIdx.x == 0) frame_counters_begin(fc, pm.n_slots);
    const bool seg_out = kPrimary && !kLoop && fc.seg_counts != nullptr;
    const bool seg_in = !kPrimary && kLoop && fc.seg_counts != nullptr;
    uint32_t count;
    if (seg_in) {
        // exclusive prefix sum of the segment sizes: thread t sums a run of consecutive segments, the runs are scanned per wave
        // (shuffles) and across waves (s_wave_count), then every thread writes the prefixes of its run
        const uint32_t per = (fc.n_segs + blockDim.x - 1u) / blockDim.x;
        const uint32_t first = threadIdx.x * per;
        uint32_t sum = 0;
        for (uint32_t j = 0; j < per; j++) if (first + j < fc.n_segs) sum += fc.seg_counts[first + j];
        uint32_t incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const uint32_t v = __shfl_up(incl, off, 64); if ((int)lane_id() >= off) incl += v; }
        if (lane_id() == 63u) s_wave_count[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) base += s_wave_count[w];
        uint32_t run = base + incl - sum;
        for (uint32_t j = 0; j < per; j++)
            if (first + j < fc.n_segs) { s_seg_prefix[first + j] = run; run += fc.seg_counts[first + j]; }
        if (threadIdx.x == blockDim.x - 1u) s_seg_prefix[fc.n_segs] = base + incl;
        __syncthreads();
        count = s_seg_prefix[fc.n_segs];
        if (blockIdx.x == 0 && threadIdx.x == 0) *const_cast<uint32_t*>(count_in_ptr) = count;  // the queue size, for the statistics and the next frame's grid estimate
    } else {
        count = kPrimary ? pm.n_slots : *count_in_ptr;
    }
    if (seg_out && threadIdx.x == 0) { s_seg_count = 0; s_seg_next = 0; s_loop_next = 0; }
    if (kIters > 1u && threadIdx.x == 0) { s_refl[0] = 0; s_refl[1] = 0; }
    if (blockIdx.x * blockDim.x >= count) {
        if (seg_out && threadIdx.x == 0) fc.seg_counts[blockIdx.x] = 0;
        return;
    }
    // Tile order.  A workgroup's waves draw its 64-slot tiles from s_seg_next; in slot order those run down the image, so every wave would
    // END on a ground tile (1 400-2 200 wave instructions against ~100 for a sky tile) and wait at the closing barrier for the slowest of
    // eight, with the wave slots of all of them held.  Over a view with beam lists the class of a tile is known beforehand -- the count word of
    // its list, 0 = every ray misses -- so the tiles with a non-empty list are drawn first and the empty ones fill the end (longest
    // processing time first, inside the workgroup; each class keeps its slot order).  The last wave of the workgroup builds the table with
    // ballots: no counter to reset, one order whatever the timing.  Its loads are issued here and used after the scene is staged.  A
    // workgroup visits fc.seg_cap / 64 tiles (those past the end of the frame count as empty: they stay the last ones drawn).  Without lists,
    // or with more tiles than the table holds, the order is the slot order.  (The table's size lives in LDS with it: the draw reads both with
    // the lane that made the atomic, and the tile loop carries nothing in registers for them.)
    // spp > 1 keeps the slot order: its primary pass is a tenth of the frame, and the 4K 16-spp frame was 3 % slower with the table.
    constexpr bool kTileOrder = kPrimary && !kLoop && !kMulti;
    const uint32_t n_tiles = (kTileOrder && seg_out && fp.beam_lists != nullptr && (fc.seg_cap >> 6) <= (fc.tile_opts & 0xFFFFu)) ? fc.seg_cap >> 6 : 0u;  // (0: no table)
    const bool tile_builder = n_tiles != 0u && (threadIdx.x >> 6) == (blockDim.x >> 6) - 1u;
    constexpr uint32_t kTileChunks = kTileTable / 64u;
    constexpr uint32_t kNoTile = ~0u;  // (a draw past the end of the table: the tiles of the workgroup are all taken)
    // Which tiles a workgroup visits.  The batch map -- draw w is wave slot w % waves of batch b + (w / waves) * gridDim.x -- is what the dense
    // hand-over needs, whose barriers keep a whole workgroup on one batch of blockDim.x slots; it gives a workgroup runs of eight consecutive
    // tiles, 17 block rows apart at 1080p, so the workgroups whose runs fall on the spheres (tiles without a region record, whose bounce-1 rays
    // walk the tree) got up to 23 such tiles against a mean of 8 (tools/tile_balance.py).  The segmented hand-over has no barrier in the tile loop: there draw w of a 1-spp
    // workgroup is tile b + gridDim.x * w, every gridDim.x-th tile of the whole frame (kTileOptInterleave; PT_TILE_INTERLEAVE=0: the batch map).
    // Both maps rise with w, so the tiles past the end of the frame are a workgroup's largest w in either.
    // Three classes where the view has region records: tiles with a list and no region first (the tree walks), then the region-served, then the
    // empty ones -- the same ballots and prefix counts, one more word loaded per tile.
    uint32_t tile_class[kTileChunks], tile_region[kTileChunks];
    if (tile_builder) {
        const uint32_t waves = blockDim.x >> 6;
        const bool interleave = (fc.tile_opts & kTileOptInterleave) != 0u;
#pragma unroll
        for (uint32_t k = 0; k < kTileChunks; k++) {
            const uint32_t w = k * 64u + lane_id();
            const uint32_t i0 = interleave ? (blockIdx.x + gridDim.x * w) << 6 : (blockIdx.x + (w / waves) * gridDim.x) * blockDim.x + (w % waves) * 64u;
            const bool inside = w < n_tiles && i0 < count;
            tile_class[k] = inside ? fp.beam_lists[(size_t)(i0 >> 6) * kBeamRecord] : 0u;
            tile_region[k] = (inside && fp.refl_lists != nullptr) ? fp.refl_lists[(size_t)(i0 >> 6) * kReflRecord] : 0u;
        }
    }
    auto build_tile_order = [&]() {
        unsigned long long heavy[kTileChunks], served[kTileChunks];
        uint32_t n_heavy = 0, n_served = 0;
#pragma unroll
        for (uint32_t k = 0; k < kTileChunks; k++) {
            heavy[k] = __ballot(tile_class[k] != 0u && tile_region[k] == 0u);
            served[k] = __ballot(tile_class[k] != 0u && tile_region[k] != 0u);
            n_heavy += __popcll(heavy[k]);
            n_served += __popcll(served[k]);
        }
        const unsigned long long below = (1ull << lane_id()) - 1ull;
        uint32_t at_heavy = 0, at_served = n_heavy, at_light = n_heavy + n_served;
#pragma unroll
        for (uint32_t k = 0; k < kTileChunks; k++) {
            const uint32_t w = k * 64u + lane_id();
            const bool h = tile_class[k] != 0u && tile_region[k] == 0u, s = tile_class[k] != 0u && tile_region[k] != 0u;
            const unsigned long long light = ~(heavy[k] | served[k]);
            const uint32_t pos = h ? at_heavy + __popcll(heavy[k] & below) : s ? at_served + __popcll(served[k] & below) : at_light + __popcll(light & below);
            if (w < n_tiles) s_tile_order[pos] = (uint16_t)w;
            at_heavy += __popcll(heavy[k]);
            at_served += __popcll(served[k]);
            at_light += __popcll(light);
        }
    };
    if (kTileOrder && seg_out && threadIdx.x == 0) s_tile_n = n_tiles;
    if (!kLds) {
        if (tile_builder) build_tile_order();
        if (seg_out || kIters > 1u) __syncthreads();  // (with kLds the barrier after stage_scene orders the reset and the table)
    }
    if (kLds) {
        stage_scene(sv, smem, false);
        if (tile_builder) build_tile_order();
        __syncthreads();
        if (kCoop && fc.coop_walk != 0u && sv.n > 1u) {
            if (threadIdx.x == 0) build_cut(smem, s_cut);
            __syncthreads();
        }
    }
    TreeWalk<StackT> tw;
    tree_walk_pointers<kLds, StackT>(sv, tw);
    const auto [nodes, sph, ids, stack] = tw;
    const uint32_t lane = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const bool coop = kCoop && fc.coop_walk != 0u && sv.n > 1u && (blockDim.x & 63u) == 0u;  // (whole waves only: every lane takes part in the exchanges)
    uint32_t my_rays = 0;
    // A share of the NEXT primary-beam lists of a moving camera (FrameParams::beam_job, pt_api.hip beam_cache_lookup): the first wave of the
    // first workgroups walks 64 blocks' pyramids each, one lane per block, before it joins its workgroup's tiles -- an 8192-block share per
    // frame hides in the pass (its other waves take the tiles meanwhile), where a whole build as a launch of its own stalled a lane for 60 us
    // and put the three lanes out of step for several frames (tools/experiments/moving_trace.sh).
    if (kPrimary && !kLoop && wave == 0) {
        const BeamJob job = cold_arg<BeamJob>(offsetof(BounceArgHead, fp) + offsetof(FrameParams, beam_job));
        const uint32_t j = blockIdx.x * 64u + lane;
        if (j < job.n_blocks) {
            CameraParams cam_b = cold_arg<CameraParams>(offsetof(BounceArgHead, fp) + offsetof(FrameParams, cam));
            cam_b.Position = make_f3(job.centre[0], job.centre[1], job.centre[2]);
            cam_b.Right = make_f3(job.right[0], job.right[1], job.right[2]);  // (the orientation the lists are made for: this frame's, or one extrapolated from a turn)
            cam_b.Up = make_f3(job.up[0], job.up[1], job.up[2]);
            cam_b.Forward = make_f3(job.forward[0], job.forward[1], job.forward[2]);
            beam_walk_block<StackT>(sv, nodes, ids, stack, blockDim.x, cold_arg<PixelMap>(offsetof(BounceArgHead, pm)), cam_b, job.slack, job.margin_px, job.first_block + j, job.lists);
        }
    }
    // Work distribution: a static grid-stride over the batches -- except for the looping pass behind a segmented hand-over,
    // where every WAVE pulls its next 64 entries from a work cursor (one atomic per 64 paths; no barrier inside this loop in
    // the looping form): a segment lists one workgroup's tiles top to bottom of the image, and a static stride over such a
    // queue can hand a workgroup the same image region again and again (C3: 7.2 vs 6.5 ms for the looping pass).
    // 1 spp (kMulti = false): every wave's FIRST 64 entries are its own by position (no atomic); only what lies beyond one entry
    // per thread of the grid is handed out by the cursor.  The host sizes the grid to the queue, so the pass makes no cursor
    // atomics at all: 1200 waves hitting one address at launch cost 5-10 us EACH (tools/experiments/loopstamps.py: same-address
    // device-scope atomics from 8 XCDs serialise), before the first ray and again to learn that the queue is empty -- the
    // driver's 20-step C2 run went from 0.102-0.106 to 0.095 ms per frame.  At spp > 1 a wave draws ~30 long batches, the atomics
    // do not show, and the extra loop state made that kernel spill (C4 +3 %): it keeps the plain cursor.
    uint32_t* const cursor = const_cast<uint32_t*>(count_in_ptr) + fc.n_counts + 1u;  // the work cursor of this queue (zeroed when the counters are folded)
    for (uint32_t base = blockIdx.x * blockDim.x;; base += gridDim.x * blockDim.x) {
        uint32_t i;
        if (seg_in) {
            uint32_t b;
            const uint32_t static_end = kMulti ? 0u : gridDim.x * blockDim.x;
            if (!kMulti && base < static_end) {  // the first pass through this loop
                b = base + wave * 64u;
            } else {
                if (!kMulti && static_end >= count) break;
                uint32_t v = 0;
                if (lane == 0) v = atomicAdd(cursor, 64u);
                b = static_end + __builtin_amdgcn_readfirstlane(v);
            }
            if (b >= count) break;
            i = b + lane;
        } else if (seg_out) {
            // the workgroup's waves take its 64-slot tiles (every gridDim.x-th tile of the frame; with the batch map those of the same strided
            // set of batches as below) from a counter in LDS: a wave that drew sky tiles moves on instead of idling behind its neighbours
            uint32_t w = 0;
            if (lane == 0) {
                w = atomicAdd(&s_seg_next, 1u);
                if (kTileOrder) {
                    const uint32_t n = s_tile_n;
                    if (n != 0u) w = w < n ? s_tile_order[w] : kNoTile;
                }
            }
            w = __builtin_amdgcn_readfirstlane(w);
            if (w == kNoTile) break;
            // (the map's switch is read where it is used, like the short path's below: one scalar load per draw, nothing carried through the body)
            if (kTileOrder && (cold_arg<uint32_t>(offsetof(BounceArgs, fc) + offsetof(FrameCounters, tile_opts)) & kTileOptInterleave) != 0u) {
                const uint32_t b = (blockIdx.x + gridDim.x * w) << 6;
                if (b >= count) break;
                i = b + lane;
            } else {
                const uint32_t waves = blockDim.x >> 6;
                const uint32_t b = (blockIdx.x + (w / waves) * gridDim.x) * blockDim.x;
                if (b >= count) break;
                i = b + (w % waves) * 64u + lane;
            }
        } else {
            if (base >= count) break;
            i = base + threadIdx.x;
        }
        bool emit = false;
        PathState ps;
        if (kCoop && kLoop && coop) {
            const bool alive = i < count;
            if (alive) {
                if (seg_in) {
                    uint32_t lo = 0, hi = fc.n_segs;
                    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_seg_prefix[mid] <= i) lo = mid; else hi = mid; }
                    ps = load_path<kDn>(qin, lo * fc.seg_cap + (i - s_seg_prefix[lo]));
                } else {
                    ps = load_path<kDn>(qin, i);
                }
            } else {
                ps.o = make_f3(0.f, 0.f, 0.f); ps.d = make_f3(0.f, 0.f, 1.f);  // (a helper from the start: the exchanges read every lane's ray registers)
            }
            coop_bounces<StackT, kDn>(sv, pm, fp, scratch, out, nodes, sph, ids, s_cut, stack, blockDim.x, ps, alive, my_rays);
            continue;  // (a looping pass hands nothing on)
        }
        // primary beams: this wave's 64 slots are one 8x8-pixel block; its candidate list was made by beam_kernel
        // (its count and first three ids in one scalar load, the first candidate's sphere in the next: both are back before the rays are made)
        ListHead beam{ nullptr, ~0u, kBeamListCap, 0u, 0u, 0u, { 0u, 0u, 0u, 0u } };
        if (kPrimary && fp.beam_lists) {
            const uint32_t* beam_rec = fp.beam_lists + (size_t)__builtin_amdgcn_readfirstlane(i >> 6) * kBeamRecord;
            const u32x4 head = scalar_load<u32x4>(beam_rec);
            beam.ids = beam_rec + 1;
            beam.count = head[0]; beam.id0 = head[1]; beam.id1 = head[2]; beam.id2 = head[3];
            beam.s0 = list_first_sphere(sv, beam.count, kBeamListCap, beam.id0);
        }
        const uint32_t beam_count = beam.count;
        // Sky tiles: an empty list says that every ray of the block misses, and a primary miss of these instances ends the pixel with one
        // store (shade_step_ex, shade_miss).  The short path stores the environment's colour in the primary direction, as primary_ray makes
        // it, and is done: no tmin / tmax, no RNG stream, no list walk, no shade_step, no second slot -> pixel mapping.
        // (spp > 1 also leaves Scratch::primary_hit on a miss and the textured instances may sample an environment map: the general path.)
        constexpr bool kSky = kPrimary && !kLoop && !kMulti && !kTex;
        // (wave-uniform, and used up before the trace: the knob's word is read from the kernarg segment only behind an empty list, and nothing of
        // this is carried through the loop's body, where the scalar registers are short)
        const bool sky = kSky && beam_count == 0u && (cold_arg<uint32_t>(offsetof(BounceArgs, fc) + offsetof(FrameCounters, tile_opts)) & kTileOptSky) != 0u;
        // the slot -> pixel mapping, once per tile: the wave's 64 slots are one 8x8 block, so the block's origin is scalar arithmetic (two
        // multiply-high quotients at most) and a lane adds its place in the block; the pixel writes of shade_step use the same origin
        // (the primary instances that also loop keep the per-lane form: with the origin's scalars live they gained scratch)
        constexpr bool kTileMap = kPrimary && !kLoop, kBlock = kTileMap && !kMulti;
        BlockOrigin bo{};
        if (kTileMap) bo = block_origin(cold_arg<PixelMap>(offsetof(BounceArgHead, pm)), (uint32_t)__builtin_amdgcn_readfirstlane(i >> 6));
        if (i < count) {
            bool live = true;
            float tmin = 0.0f, tmax = kInf;
            if (kPrimary) {
                const PixelRef pr = kTileMap ? block_pixel(bo, i & 63u) : slot_to_pixel(cold_arg<PixelMap>(offsetof(BounceArgHead, pm)), i);
                live = pr.valid;
                ps.slot = i; ps.bounce = 0; ps.sample = 0; ps.dirty = false; ps.via_t = false; ps.dn_spec = false; ps.rng = 0;
                ps.T = make_f3(1.f, 1.f, 1.f);
                ps.o = make_f3(0.f, 0.f, 0.f); ps.d = make_f3(0.f, 0.f, 1.f);
                if (live) {
                    const CameraParams cam_c = cold_arg<CameraParams>(offsetof(BounceArgHead, fp) + offsetof(FrameParams, cam));
                    ps.o = cam_c.Position;
                    ps.d = primary_dir(cam_c, pr.px, pr.py);
                    if (kSky && sky) {
                        const f3 env = environment_color(sv.env[0], sv.env[1], sv.env[2], sv.env[3], ps.d);
                        out[pr.out_index] = make_float4(env.x, env.y, env.z, 1.0f);
                    } else {
                        primary_range(cam_c, ps.d, tmin, tmax);  // (the division is the traced tiles' alone: a sky tile reads no tmin / tmax)
                        ps.rng = rng_init(pr.px, pr.py, fp.frame_index);
                    }
                } else if (cold_arg<uint32_t>(offsetof(BounceArgHead, pm) + offsetof(PixelMap, mode)) == 1u) {
                    out[pr.out_index] = make_float4(0.f, 0.f, 0.f, 0.f);  // padding pixel of an edge tile
                }
                if (kSky && sky) live = false;
            } else if (seg_in) {
                // dense index -> (segment, offset): the last segment whose prefix is <= i
                uint32_t lo = 0, hi = fc.n_segs;
                while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_seg_prefix[mid] <= i) lo = mid; else hi = mid; }
                ps = load_path<kDn>(qin, lo * fc.seg_cap + (i - s_seg_prefix[lo]));
            } else {
                ps = load_path<kDn>(qin, i);
            }
            constexpr bool kMerged = kLoop && kMulti && !kPrimary;  // (shade_step_ex: one pass through the surface code per iteration)
            if (kMerged) {
                constexpr int kCacheMode = kTex ? 0 : 2;
                bool pending = false;
                for (;;) {
                    float t = 0.0f;
                    uint32_t id = kMissId;
                    if (!pending) closest_hit_any<kLds, StackT, kTex>(sv, nodes, sph, ids, ps.o, ps.d, 0.0f, kInf, stack, blockDim.x, t, id);
                    const int r = shade_step_ex<true, kTex, false, kCacheMode, true, kDn>(sv, pm, fp, scratch, out, ps, t, id, pending);
                    if (r == kShadeDone) break;
                    pending = r == kShadePending;
                    if (!pending) my_rays++;  // a ray spawned and traced inside this kernel
                }
            } else if (live) {
                bool primary_trace = kPrimary;
                uint32_t iter = 0;
                for (;;) {
                    float t;
                    uint32_t id;
                    if (kPrimary && primary_trace && fp.beam_lists && beam_count <= kBeamListCap) {
                        closest_hit_list<kTex>(sv, beam, ps.o, ps.d, tmin, tmax, t, id);
                        if (kMulti) scratch.primary_hit[i] = make_uint2(as_uint(t), id);
                    } else {
                        // reflection beams: the in-register first bounce of a block with a region record, when every active lane's ray lies in the region
                        // (the counts of pt_get_refl_stats are kept only while the records are in use: a frame without them runs nothing but the pointer test)
                        bool listed = false;
                        ListHead refl{ nullptr, 0u, kReflListCap, 0u, 0u, 0u, { 0u, 0u, 0u, 0u } };
                        if (kIters > 1u && !primary_trace && fp.refl_lists) {
                            // the record's first sixteen words in one scalar round trip: the count, the region's ten words and the first five ids
                            static_assert(kReflIds == 11u && kReflRecord == 32u, "the region record's layout");
                            const uint32_t* rrec = fp.refl_lists + (size_t)__builtin_amdgcn_readfirstlane(i >> 6) * kReflRecord;
                            const u32x8 h0 = scalar_load<u32x8>(rrec), h1 = scalar_load<u32x8>(rrec + 8);
                            refl.ids = rrec + kReflIds;
                            refl.count = h0[0]; refl.id0 = h1[3]; refl.id1 = h1[4]; refl.id2 = h1[5];
                            refl.s0 = list_first_sphere(sv, refl.count, kReflListCap, refl.id0);
                            listed = refl.count != 0u && __ballot(!refl_contains(h0, h1, ps.o, ps.d)) == 0ull;
                            if (lane == (uint32_t)__builtin_amdgcn_readfirstlane(lane)) { atomicAdd(&s_refl[0], 1u); if (listed) atomicAdd(&s_refl[1], 1u); }
                        }
                        if (listed) closest_hit_list<kTex>(sv, refl, ps.o, ps.d, tmin, tmax, t, id);
                        else closest_hit_any<kLds, StackT, kTex>(sv, nodes, sph, ids, ps.o, ps.d, tmin, tmax, stack, blockDim.x, t, id);
                        if (kMulti && kPrimary && primary_trace) scratch.primary_hit[i] = make_uint2(as_uint(t), id);
                    }
                    primary_trace = false;
                    // Scratch::primary_cache: the compacting primary pass of an spp > 1 frame writes the records, the looping pass restarts samples from them
                    constexpr int kCacheMode = (kMulti && !kTex) ? ((kPrimary && !kLoop) ? 1 : ((kLoop && !kPrimary) ? 2 : 0)) : 0;
                    if (kDI)  // row N4: the first shading of the primary surface also makes its direct-illumination estimate
                        emit = shade_step<kMulti, kTex, true, kCacheMode, kDn, kBlock>(sv, pm, fp, scratch, out, ps, t, id,
                                                              [&](f3 so, f3 sd, float& t2, uint32_t& id2) { closest_hit_any<kLds, StackT, kTex>(sv, nodes, sph, ids, so, sd, 0.0f, kInf, stack, blockDim.x, t2, id2); },
                                                              &my_rays, kBlock ? &bo : nullptr);
                    else
                        emit = shade_step<kMulti, kTex, false, kCacheMode, kDn, kBlock>(sv, pm, fp, scratch, out, ps, t, id, NoTrace(), nullptr, kBlock ? &bo : nullptr);
                    if (!emit) break;
                    if (!kLoop && ++iter >= kIters) break;
                    my_rays++;  // a ray spawned and traced inside this kernel (queued rays are counted by counts[])
                    tmin = 0.0f; tmax = kInf;
                }
            }
        }
        if (seg_out) {
            // Segmented hand-over: the wave reserves room in the workgroup's own segment with ONE LDS atomic; no barrier -- the
            // waves of a workgroup no longer wait for its slowest wave after every batch (the barriers of the dense form below
            // cost 18 % of the primary pass at C2: 132 -> 109 us measured with the compaction compiled out).
            const unsigned long long mask = __ballot(emit);
            const uint32_t wave_n = __popcll(mask);
            if (wave_n == 0u) continue;  // (nothing to hand over: a sky tile, a tile whose paths all ended)
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&s_seg_count, wave_n);
            base = __shfl(base, 0, 64);
            if (emit) store_path<kDn>(qout, blockIdx.x * fc.seg_cap + base + __popcll(mask & ((1ull << lane) - 1ull)), ps);
        } else if (!kLoop) {
            // One atomic per WORKGROUP.  (One per wave -- no barriers, waves never wait for each other -- was measured and is
            // far worse: 0.116 -> 0.201 ms per C2 frame; 8x as many same-address device-scope atomics from 8 XCDs serialise.)
            const unsigned long long mask = __ballot(emit);
            const uint32_t wave_n = __popcll(mask);
            const uint32_t prefix = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) s_wave_count[wave] = wave_n;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t total = 0;
                const uint32_t n_waves = blockDim.x >> 6;
                for (uint32_t w = 0; w < n_waves; w++) { const uint32_t c = s_wave_count[w]; s_wave_count[w] = total; total += c; }
                s_block_base = total ? atomicAdd(count_out_ptr, total) : 0u;
            }
            __syncthreads();
            if (emit) store_path<kDn>(qout, s_block_base + s_wave_count[wave] + prefix, ps);
            __syncthreads();
        }
    }
    uint32_t my_loop_rays = 0;
    if (seg_out) {
        __syncthreads();  // (also orders the queue records written above before the reads below, workgroup scope)
        const uint32_t n_own = s_seg_count;
        if (threadIdx.x == 0) {
            fc.seg_counts[blockIdx.x] = n_own;
            if (kFuse && n_own) atomicAdd(count_out_ptr, n_own);  // the queue size, for the statistics
        }
        if (kFuse) {
            // Fused form: the workgroup finishes the paths of its OWN segment -- no second launch, no dependency on any other
            // workgroup; workgroups that are done with their primary tiles run these latency-bound tails while others still trace
            // primaries.  Waves take 64 entries at a time from a counter in LDS.
            for (;;) {
                uint32_t w = 0;
                if (lane == 0) w = atomicAdd(&s_loop_next, 64u);
                w = __builtin_amdgcn_readfirstlane(w);
                if (w >= n_own) break;
                const uint32_t i = w + lane;
                if (kCoop && coop) {
                    PathState ps;
                    if (i < n_own) ps = load_path<kDn>(qout, blockIdx.x * fc.seg_cap + i);
                    else { ps.o = make_f3(0.f, 0.f, 0.f); ps.d = make_f3(0.f, 0.f, 1.f); }
                    coop_bounces<StackT, kDn>(sv, pm, fp, scratch, out, nodes, sph, ids, s_cut, stack, blockDim.x, ps, i < n_own, my_loop_rays);
                } else if (i < n_own) {
                    PathState ps = load_path<kDn>(qout, blockIdx.x * fc.seg_cap + i);
                    for (;;) {
                        float t;
                        uint32_t id;
                        closest_hit_any<kLds, StackT, kTex>(sv, nodes, sph, ids, ps.o, ps.d, 0.0f, kInf, stack, blockDim.x, t, id);
                        if (!shade_step<kMulti, kTex, false, 0, kDn>(sv, pm, fp, scratch, out, ps, t, id)) break;
                        my_loop_rays++;
                    }
                }
            }
        }
    }
    if (kLoop || kIters > 1u || kFuse || kDI) {
        // rays traced in registers: wave reduce, then ONE atomic pair per workgroup (same-address device-scope atomics from
        // 8 XCDs serialise: one per wave made the non-persistent form of this kernel three times slower)
        unsigned long long total = my_rays, total2 = kFuse ? my_loop_rays : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            total += __shfl_down(total, off, 64);
            if (kFuse) total2 += __shfl_down(total2, off, 64);
        }
        __shared__ uint32_t s_wave_count2[kFusedThreads / 64];
        __syncthreads();  // s_wave_count is free again
        if (lane == 0) { s_wave_count[wave] = (uint32_t)total; if (kFuse) s_wave_count2[wave] = (uint32_t)total2; }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long sum = 0, sum2 = 0;
            for (uint32_t w = 0; w < (blockDim.x >> 6); w++) { sum += s_wave_count[w]; if (kFuse) sum2 += s_wave_count2[w]; }
            if (sum + sum2) atomicAdd(fc.tail_rays, sum + sum2);
            if (sum && !kLoop && !kDI) atomicAdd(fc.totals + 4, sum);  // running count of the rays a primary pass traced in registers (statistics)
            if (kIters > 1u && s_refl[0]) { atomicAdd(fc.totals + 8, (unsigned long long)s_refl[0]); if (s_refl[1]) atomicAdd(fc.totals + 9, (unsigned long long)s_refl[1]); }
        }
    }
}

// Launches the bounce_kernel instance for (kLds, StackT) that the run-time switches select.  One translation unit per
// (kLds, StackT) pair instantiates this (pt_bounce_*.hip); launch_bounce (pt_kernels.hip) picks the pair.
template <bool kLds, typename StackT>
hipError_t launch_bounce_for(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const RayQueue& qin, const RayQueue& qout,
                             const Scratch& scratch, float4* out, const uint32_t* count_in, uint32_t* count_out, const FrameCounters& fc,
                             bool primary, bool loop, bool inline2, uint32_t threads, uint32_t grid, hipStream_t stream)
{
    const uint32_t lds = traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, sv.lds_scene != 0, threads);
    hipError_t err = hipSuccess;
#define PT_BOUNCE9(P, LP, M, X, I, F, D, N) \
    err = launch_kernel(bounce_kernel<kLds, StackT, P, LP, M, X, I, F, D, N>, grid, threads, lds, stream, sv, pm, fp, qin, qout, scratch, out, count_in, count_out, fc)
/* row N7: a denoiser frame (scratch.dn.mode != 0) runs the kDn instance of the same schedule */
#define PT_BOUNCE8(P, LP, M, X, I, F, D)                                                                                   \
    do { if (scratch.dn.mode) PT_BOUNCE9(P, LP, M, X, I, F, D, true); else PT_BOUNCE9(P, LP, M, X, I, F, D, false); } while (0)
/* the direct-illumination estimate (row N4) is made by the compacting primary pass, unless the caller supplied it (pt_render_with_di) */
#define PT_BOUNCE7(P, LP, M, X, I, F)                                                                                      \
    do { if (fp.di_enabled && fp.di_enabled != kDiExternal && P && !LP) PT_BOUNCE8(P, LP, M, X, I, F, (P && !LP)); else PT_BOUNCE8(P, LP, M, X, I, F, false); } while (0)
/* the fused form (the primary pass finishes its own segments) exists only for the compacting primary pass */
#define PT_BOUNCE6(P, LP, M, X, I)                                                                                         \
    do { if (fc.fuse_loop && P && !LP) PT_BOUNCE7(P, LP, M, X, I, (P && !LP)); else PT_BOUNCE7(P, LP, M, X, I, false); } while (0)
/* the in-register second bounce exists only for the 1-spp compacting primary pass */
#define PT_BOUNCE5(P, LP, M, X)                                                                                            \
    do { if (inline2 && P && !LP && !M) PT_BOUNCE6(P, LP, M, X, (P && !LP && !M)); else PT_BOUNCE6(P, LP, M, X, false); } while (0)
#define PT_BOUNCE4(P, LP, M)                                                                                               \
    do { if (sv.tex_maps) PT_BOUNCE5(P, LP, M, true); else PT_BOUNCE5(P, LP, M, false); } while (0)
#define PT_BOUNCE3(P, LP)                                                                                                  \
    do { if (fp.spp > 1) PT_BOUNCE4(P, LP, true); else PT_BOUNCE4(P, LP, false); } while (0)
    if (primary) { if (loop) PT_BOUNCE3(true, true); else PT_BOUNCE3(true, false); }
    else { if (loop) PT_BOUNCE3(false, true); else PT_BOUNCE3(false, false); }
#undef PT_BOUNCE3
#undef PT_BOUNCE4
#undef PT_BOUNCE5
#undef PT_BOUNCE6
#undef PT_BOUNCE7
#undef PT_BOUNCE8
#undef PT_BOUNCE9
    return err;
}

// the three instantiations (pt_bounce_lds16.hip, pt_bounce_g16.hip, pt_bounce_g32.hip).  An LDS-resident tree has fewer than
// 32767 nodes (64 KB hold ~700 spheres), so <true, uint32_t> does not exist.
#define PT_BOUNCE_LAUNCHER_ARGS const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const RayQueue& qin, const RayQueue& qout, const Scratch& scratch, \
    float4* out, const uint32_t* count_in, uint32_t* count_out, const FrameCounters& fc, bool primary, bool loop, bool inline2, uint32_t threads, uint32_t grid, hipStream_t stream
hipError_t launch_bounce_lds16(PT_BOUNCE_LAUNCHER_ARGS);
hipError_t launch_bounce_g16(PT_BOUNCE_LAUNCHER_ARGS);
hipError_t launch_bounce_g32(PT_BOUNCE_LAUNCHER_ARGS);

}  // namespace pt
