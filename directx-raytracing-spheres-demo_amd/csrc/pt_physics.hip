// pt_physics.hip -- the kernels of row N23 (pt_physics_*, DESIGN.md spec S27) over pt_physics.h:
//   forces     one lane per body: v += h a(x); copies the velocities the step started from and the pre-solve velocity, clears the count
//   pairs      one lane per walking body: its box against the tree (the LDS copy and the 16-bit stack below 32767 nodes, global memory
//              and the 32-bit stack above: with_tree_walk), every leaf it meets through ph_walker_handles and ph_contact; kCount counts
//              the contacts of both bodies, else ph_pair_impulse goes to both bodies' accumulators
//   large      the pairs of two bodies of the LARGE list, brute force: one lane per ordered pair (at most 64 x 64)
//   apply      one lane per body: accumulators -> velocities, cleared
//   integrate  one lane per body: ph_integrate, or the freeze
// Accumulators and counters take integer atomics whose result is not read (global_atomic_add_x2 / global_atomic_add without return).
#include "pt_trace.h"
#include "pt_physics.h"

namespace pt {

namespace {

constexpr uint32_t kPhThreads = 256;

__device__ __forceinline__ void ph_add(long long* acc, long long v)
{
    if (v != 0) (void)atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);
}

// one contact: the count of both bodies, or the impulse of one iteration into both bodies' accumulators; lo < hi
template <bool kCount>
__device__ __forceinline__ void ph_pair(const PhDevice& d, const PhParams& p, uint32_t lo, uint32_t hi, PhVec4 slo, PhVec4 shi, PtPhysicsBody blo, PtPhysicsBody bhi,
                                        uint32_t& contacts, bool& clamped)
{
    if (kCount) {
        f3 n;
        float pen;
        if (!ph_contact(slo, shi, n, pen)) return;
        (void)atomicAdd(d.count + lo, 1u);
        (void)atomicAdd(d.count + hi, 1u);
        contacts++;
    } else {
        PhPair q;
        q.sa = slo; q.sb = shi;
        q.va = ph_xyz(d.vel[lo]); q.vb = ph_xyz(d.vel[hi]);
        q.wa = ph_xyz(d.ang[lo]); q.wb = ph_xyz(d.ang[hi]);
        q.v0a = ph_xyz(d.v0[lo]); q.v0b = ph_xyz(d.v0[hi]);
        q.ima = blo.InvMass; q.imb = bhi.InvMass;
        q.na = d.count[lo]; q.nb = d.count[hi];
        PhImpulse r;
        if (!ph_pair_impulse(q, p, r)) return;
        long long* a = d.acc + (size_t)lo * kPhAccPerBody;
        long long* b = d.acc + (size_t)hi * kPhAccPerBody;
        ph_add(a + 0, ph_quantize(r.dva.x, clamped)); ph_add(a + 1, ph_quantize(r.dva.y, clamped)); ph_add(a + 2, ph_quantize(r.dva.z, clamped));
        ph_add(a + 3, ph_quantize(r.dwa.x, clamped)); ph_add(a + 4, ph_quantize(r.dwa.y, clamped)); ph_add(a + 5, ph_quantize(r.dwa.z, clamped));
        ph_add(b + 0, ph_quantize(r.dvb.x, clamped)); ph_add(b + 1, ph_quantize(r.dvb.y, clamped)); ph_add(b + 2, ph_quantize(r.dvb.z, clamped));
        ph_add(b + 3, ph_quantize(r.dwb.x, clamped)); ph_add(b + 4, ph_quantize(r.dwb.y, clamped)); ph_add(b + 5, ph_quantize(r.dwb.z, clamped));
    }
}

__device__ __forceinline__ void ph_report(const PhDevice& d, uint32_t contacts, bool clamped)
{
    if (contacts) (void)atomicAdd(d.report + 0, contacts);
    if (clamped) (void)atomicOr(d.report + 1, 1u);
}

__global__ __launch_bounds__(kPhThreads) void physics_forces_kernel(PhDevice d, PhParams p)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const PtPhysicsBody b = d.body[i];
    PhVec4 v = d.vel[i];
    d.vel_start[i] = v;
    d.ang_start[i] = d.ang[i];
    const f3 a = ph_acceleration(d.sph, i, b, p);
    v.x = v.x + p.h * a.x; v.y = v.y + p.h * a.y; v.z = v.z + p.h * a.z;
    d.vel[i] = v;
    d.v0[i] = v;
    d.count[i] = 0u;
}

// A leaf box holds its sphere's box and the refit's padding (2^-17 of the largest coordinate), and ph_contact's distance is below the sum
// of the radii only where the two spheres' boxes overlap up to a few roundings: every partner in contact is met, whatever the tree.
template <bool kLds, typename StackT, bool kCount>
__global__ __launch_bounds__(kTraverseThreads) void physics_pairs_kernel(SceneView sv, PhDevice d, PhParams p)
{
    TreeWalk<StackT> tw;
    tree_walk_setup<kLds, StackT>(sv, tw);
    const float4* __restrict__ nodes = tw.nodes;
    const float4* __restrict__ sorted = tw.sph;
    const uint32_t* __restrict__ ids = tw.ids;
    StackT* stack = tw.stack;
    const uint32_t stride = blockDim.x;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const PtPhysicsBody bi = d.body[i];
    if (bi.Flags & (PT_PHYSICS_DISABLED | kPhNoWalk)) return;
    const PhVec4 si = d.sph[i];
    const float lx = si.x - si.w, ly = si.y - si.w, lz = si.z - si.w, hx = si.x + si.w, hy = si.y + si.w, hz = si.z + si.w;
    uint32_t contacts = 0;
    bool clamped = false;
    int node = 0;
    uint32_t sp = 0;
    for (;;) {
        while (node >= 0) {
            const float4 n0 = nodes[node * 4 + 0];
            const float4 n1 = nodes[node * 4 + 1];
            const float4 n2 = nodes[node * 4 + 2];
            const float4 n3 = nodes[node * 4 + 3];
            // child 0: lo = (n0.x,n0.y,n0.z) hi = (n0.w,n1.x,n1.y); child 1: lo = (n1.z,n1.w,n2.x) hi = (n2.y,n2.z,n2.w)
            const bool h0 = lx <= n0.w && hx >= n0.x && ly <= n1.x && hy >= n0.y && lz <= n1.y && hz >= n0.z;
            const bool h1 = lx <= n2.y && hx >= n1.z && ly <= n2.z && hy >= n1.w && lz <= n2.w && hz >= n2.x;
            const int c0 = __builtin_bit_cast(int, n3.x), c1 = __builtin_bit_cast(int, n3.y);
            if (h0 && h1) {
                stack[sp] = stack_encode<StackT>(c1);
                sp += stride;
                node = c0;
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
        }
        if (node == kTraversalDone) break;
        {
            const uint32_t k = ~(uint32_t)node;
            const uint32_t j = ids[k] & kIdMask;
            if (j != i) {
                const float4 s = sorted[k];
                const PhVec4 sj = { s.x, s.y, s.z, s.w };
                const PtPhysicsBody bj = d.body[j];
                if (!(bj.Flags & PT_PHYSICS_DISABLED) && ph_walker_handles(si.w, i, sj.w, j, !(bj.Flags & kPhNoWalk))) {
                    if (i < j) ph_pair<kCount>(d, p, i, j, si, sj, bi, bj, contacts, clamped);
                    else ph_pair<kCount>(d, p, j, i, sj, si, bj, bi, contacts, clamped);
                }
            }
        }
        if (sp == 0) break;
        sp -= stride;
        node = stack_decode(stack[sp]);
    }
    ph_report(d, contacts, clamped);
}

template <bool kCount>
__global__ __launch_bounds__(kPhThreads) void physics_large_kernel(PhDevice d, PhParams p)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d.n_large * d.n_large) return;
    const uint32_t a = t / d.n_large, b = t % d.n_large;
    if (a >= b) return;
    uint32_t lo = d.large[a], hi = d.large[b];
    if (lo > hi) { const uint32_t x = lo; lo = hi; hi = x; }
    const PtPhysicsBody blo = d.body[lo], bhi = d.body[hi];
    if ((blo.Flags | bhi.Flags) & PT_PHYSICS_DISABLED) return;
    uint32_t contacts = 0;
    bool clamped = false;
    ph_pair<kCount>(d, p, lo, hi, d.sph[lo], d.sph[hi], blo, bhi, contacts, clamped);
    ph_report(d, contacts, clamped);
}

__global__ __launch_bounds__(kPhThreads) void physics_apply_kernel(PhDevice d)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    long long* a = d.acc + (size_t)i * kPhAccPerBody;
    long long q[kPhAccPerBody];
    bool any = false;
    for (uint32_t k = 0; k < kPhAccPerBody; k++) { q[k] = a[k]; any = any || q[k] != 0; }
    if (!any) return;
    PhVec4 v = d.vel[i], w = d.ang[i];
    v.x = ph_apply(v.x, q[0]); v.y = ph_apply(v.y, q[1]); v.z = ph_apply(v.z, q[2]);
    w.x = ph_apply(w.x, q[3]); w.y = ph_apply(w.y, q[4]); w.z = ph_apply(w.z, q[5]);
    d.vel[i] = v;
    d.ang[i] = w;
    for (uint32_t k = 0; k < kPhAccPerBody; k++) a[k] = 0;
}

__global__ __launch_bounds__(kPhThreads) void physics_integrate_kernel(PhDevice d, PhParams p)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const PtPhysicsBody b = d.body[i];
    if (b.Flags & PT_PHYSICS_DISABLED) return;
    PhVec4 s = d.sph[i], r = d.rot[i];
    if (ph_integrate(s, r, ph_xyz(d.vel[i]), ph_xyz(d.ang[i]), p.h)) {
        d.sph[i] = s;
        d.rot[i] = r;
    } else {  // the freeze: the state the step started from, DISABLED from now on
        d.vel[i] = d.vel_start[i];
        d.ang[i] = d.ang_start[i];
        d.body[i].Flags = b.Flags | PT_PHYSICS_DISABLED;
        (void)atomicAdd(d.report + 2, 1u);
    }
}

uint32_t blocks_for(uint32_t n) { return (n + kPhThreads - 1u) / kPhThreads; }

}  // namespace

hipError_t launch_physics_forces(const PhDevice& d, const PhParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(physics_forces_kernel, dim3(blocks_for(d.n)), dim3(kPhThreads), 0, stream, d, p);
    return hipGetLastError();
}

hipError_t launch_physics_pairs(const SceneView& sv, const PhDevice& d, const PhParams& p, bool count, hipStream_t stream)
{
    const hipError_t e = with_tree_walk(sv, [&]<bool kLds, typename StackT>() {
        return with_flag(count, [&]<bool kCount>() {
            const uint32_t threads = traverse_threads(kLds);
            return launch_kernel(physics_pairs_kernel<kLds, StackT, kCount>, (d.n + threads - 1u) / threads, threads,
                                 traverse_lds_bytes_for(sv.n_nodes, sv.n, sv.stack_depth, kLds), stream, sv, d, p);
        });
    });
    if (e != hipSuccess || d.n_large < 2u) return e;
    return with_flag(count, [&]<bool kCount>() {
        hipLaunchKernelGGL(physics_large_kernel<kCount>, dim3(blocks_for(d.n_large * d.n_large)), dim3(kPhThreads), 0, stream, d, p);
        return hipGetLastError();
    });
}

hipError_t launch_physics_apply(const PhDevice& d, hipStream_t stream)
{
    hipLaunchKernelGGL(physics_apply_kernel, dim3(blocks_for(d.n)), dim3(kPhThreads), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_physics_integrate(const PhDevice& d, const PhParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(physics_integrate_kernel, dim3(blocks_for(d.n)), dim3(kPhThreads), 0, stream, d, p);
    return hipGetLastError();
}

}  // namespace pt
