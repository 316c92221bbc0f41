// pt_sharc.h -- the radiance cache of row N14 (pt_render_sharc, DESIGN.md spec S20): a stand-in for the SHARC library the reference's
// default frame runs (Raytracing::Render(..., SHARC&, SHARCSettings), Source/Raytracing.ixx:114-148; the SHARC_UPDATE and SHARC_QUERY
// permutations of Shaders/Raytracing.hlsl:103-375; the resolve of Shaders/SHARC.hlsl:35-57).  SharcCommon.h / HashGridCommon.h are a
// submodule the reference tree does not contain: this header follows the reference's call sites and the library's published structure,
// and its arithmetic is the spec's.  Everything here compiles on the device (pt_sharc.hip) and as host C++ (the bit-parity tests):
//   sh_grid_level / sh_voxel_size / sh_key   the hash grid
//   sh_find / sh_insert                      the hash map: buckets of kShBucket keys, find-then-claim, no loop waits on another lane
//   sh_add / sh_resolve_slot                 the voxel: 32-bit integer sums (order-independent), the per-frame resolve
//   sh_update_path                           one path of the sparse update pass
//   sh_query_pixel                           one pixel of the frame: pt_render's loop with the cache look-up in it
//   sh_update_path_ex / sh_query_pixel_ex    the same two with the extras of pt_render_sharc_ex (row N18, spec S24): the frame's direct
//                                            illumination read from the caller's buffers, the denoiser outputs of spec S13 written
//   sh_resolve_slot_ff / sh_propagate_ff     the anti-firefly filter (row N19, spec S25; IsAntiFireflyEnabled through pt_render_sharc_ex): a
//                                            luminance clamp of the frame's sums against the voxel's history in front of the resolve's
//                                            join, and a weight threshold that stops the update's back-propagation.  The library's
//                                            structure as far as recollection goes; the arithmetic and the constants are this project's
// The closest-hit query is a functor trace(o, d, tmin, tmax, t, id), the surface a functor material(id, o, d, t, primary) -> HitMaterial,
// the radiance of a ray that left the scene a functor env(d).  A trace that misses returns id = 0xFFFFFFFF and t = tmax.
//
// Out of scope: the compaction pass and its HashCopyOffset buffer (SHARC.hlsl:58-61: a hole an eviction leaves is reused by the next
// insert instead); re-loading the update path's first vertex from a G-buffer (the path traces its own primary ray).
#pragma once

#include "pt_surface.h"

#if defined(__HIPCC__)
#define PT_SH_UNROLL _Pragma("unroll")
#else
#define PT_SH_UNROLL
#endif

namespace pt {

constexpr uint32_t kShBucket = 16;             // keys per bucket: 128 B, one L2 line
constexpr int kShLevelBias = 2;                // HASH_GRID_LEVEL_BIAS; the logarithm base is 2
constexpr float kShRadianceScale = 1024.0f;    // fixed point: round(x * scale)
constexpr float kShMaxContribution = 256.0f;   // a component above this (inf included) is clamped to it before quantisation
constexpr uint32_t kShPropagationDepth = 4;    // a vertex feeds itself and the kShPropagationDepth - 1 vertices before it
constexpr uint32_t kShNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kShSampleBits = 16, kShFrameBits = 8;  // voxel.w = samples | frames << 16 | stale << 24
constexpr uint32_t kShMaxSamples = (1u << kShSampleBits) - 1u, kShMaxFrames = 255u, kShMaxStale = 254u;
constexpr uint32_t kShDefaultCapacity = 1u << 22, kShDefaultDownscale = 4, kShDefaultAccumulationFrames = 10, kShDefaultMaxStaleFrames = 64;
constexpr float kShDefaultSceneScale = 50.0f;
// the anti-firefly filter (spec S25; this project's constants)
constexpr uint32_t kShFfMinSamples = 8, kShFfMinFrames = 2;  // the history the resolve's clamp needs: resolved samples, resolved frames
constexpr float kShFfFloor = 1.0f;                           // the history's luminance counts at least this
constexpr float kShFfClampBase = 5.0f, kShFfClampSlope = 5.0f;  // K = base + slope / samples: 5 for a long history, at most 5.625
constexpr float kShFfWeightThreshold = 2.0f;                 // the back-propagation stops where the running weight's luminance exceeds this

struct alignas(16) ShKeyPair { uint64_t k[2]; };  // two keys per 128-bit load

struct ShGrid {
    f3 cam_pos;
    float scene_scale;
};

struct ShMap {
    uint64_t* keys;    // capacity keys, 0 = empty
    uint4* accum;      // this frame's accumulators: fixed-point RGB sums, sample count
    uint4* resolved;   // the previous frame's resolved voxels: sums, samples | frames << 16 | stale << 24
    uint32_t capacity; // a power of two, at least kShBucket
};

struct ShFrame {
    CameraParams cam;       // the frame's camera (query), or the update grid's: InvW / InvH of the grid, jitter set per path
    uint32_t frame_index, bounces, spp, rr_enabled;
    float throughput_threshold, inv_spp;
    float roughness_threshold;  // update
    uint32_t visualize;         // query: IsHashGridVisualizationEnabled
    // pt_render_sharc_ex (spec S24), read by the _ex functions only; all zero = off
    const float4* di_diffuse;   // the frame's direct illumination, DI = Diffuse.rgb + Specular.rgb; null = none.  Update: one texel per
    const float4* di_specular;  // pixel of the di_w x di_h frame, row-major; query: indexed like `out`
    uint32_t di_w, di_h;        // update: RenderSize
    uint32_t dn_mode;           // query: 0 Denoiser::None, 1 DLSSRayReconstruction, 2 NRDReBLUR, 3 NRDReLAX
    float* spec_hit_dist;       // query, mode 1; indexed like `out`, as the next two
    float4* dn_diffuse;         // query, modes 2 / 3
    float4* dn_specular;
};

// ---------------------------------------------------------------------------------------------------- hash grid
// level = clamp(floor(log2(d2) / 2) + bias, 1, 1023), the logarithm from the exponent bits: floor(log2(d2) / 2) = e >> 1 for d2 = m 2^e
PT_HD uint32_t sh_grid_level(float dist2)
{
    const int e = (int)((as_uint(dist2) >> 23) & 0xFFu) - 127;  // (zero and denormals: -127; the sign bit of a squared length is clear)
    const int level = (e >> 1) + kShLevelBias;
    return (uint32_t)(level < 1 ? 1 : (level > 1023 ? 1023 : level));
}

// voxelSize = 2^level / (SceneScale 2^bias)
PT_HD float sh_voxel_size(uint32_t level, float scene_scale)
{
    const float p = level <= 127u ? as_float((level + 127u) << 23) : kInf;
    return p / (scene_scale * (float)(1 << kShLevelBias));
}

PT_HD float sh_dist2(f3 P, f3 cam) { const f3 v = P - cam; return dot(v, v); }

// floor(x / voxelSize) as a 17-bit two's complement field (clamped to the field's range; NaN -> the lowest cell)
PT_HD uint64_t sh_cell(float x, float voxel)
{
    float g = pt_floor(x / voxel);
    g = !(g > -65536.0f) ? -65536.0f : (g > 65535.0f ? 65535.0f : g);
    return (uint64_t)((uint32_t)(int)g & 0x1FFFFu);
}

// bits 0-16, 17-33, 34-50: the cell; 51-60: the level; 61-63: the sign octant of the front flat normal (bit set: component < 0).
// The level is at least 1, so the key is never 0 (empty): the level field is the tag.
PT_HD uint64_t sh_key(f3 P, f3 front_normal, uint32_t level, float voxel)
{
    level = level < 1u ? 1u : (level > 1023u ? 1023u : level);
    const uint64_t oct = (front_normal.x < 0.0f ? 1u : 0u) | (front_normal.y < 0.0f ? 2u : 0u) | (front_normal.z < 0.0f ? 4u : 0u);
    return sh_cell(P.x, voxel) | (sh_cell(P.y, voxel) << 17) | (sh_cell(P.z, voxel) << 34) | ((uint64_t)level << 51) | (oct << 61);
}

PT_HD uint64_t sh_key_at(const ShGrid& g, f3 P, f3 front_normal, float& voxel)
{
    const uint32_t level = sh_grid_level(sh_dist2(P, g.cam_pos));
    voxel = sh_voxel_size(level, g.scene_scale);
    return sh_key(P, front_normal, level, voxel);
}

PT_HD uint32_t sh_bucket_base(uint64_t key, uint32_t capacity)
{
    const uint32_t h = hash32((uint32_t)key ^ hash32((uint32_t)(key >> 32)));
    return (h & (capacity / kShBucket - 1u)) * kShBucket;
}

// ---------------------------------------------------------------------------------------------------- hash map
// the whole bucket is scanned (an eviction may have left holes in front of the key)
PT_HD uint32_t sh_find(const uint64_t* keys, uint32_t capacity, uint64_t key)
{
    const uint32_t base = sh_bucket_base(key, capacity);
    const ShKeyPair* pairs = reinterpret_cast<const ShKeyPair*>(keys + base);
    uint32_t found = kShNoSlot;
    for (uint32_t i = 0; i < kShBucket / 2u; i++) {
        const ShKeyPair p = pairs[i];
        if (p.k[0] == key) found = base + 2u * i;
        if (p.k[1] == key) found = base + 2u * i + 1u;
    }
    return found;
}

// 0 -> key if the slot is empty; returns what the slot held
PT_HD uint64_t sh_claim(uint64_t* slot, uint64_t key)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(reinterpret_cast<unsigned long long*>(slot), 0ull, (unsigned long long)key);
#else
    const uint64_t old = *slot;
    if (old == 0u) *slot = key;
    return old;
#endif
}

// find, then claim: one walk of the bucket in order, one compare-and-swap per slot seen empty; the slot is taken if it held 0 or the
// key itself (another lane claimed it for the same key), else the walk goes on.  kShNoSlot: the bucket is full.
// Within a launch a slot only changes from 0 to a key, every inserter of a key walks the same order, so a key never takes two slots.
PT_HD uint32_t sh_insert(uint64_t* keys, uint32_t capacity, uint64_t key)
{
    const uint32_t found = sh_find(keys, capacity, key);
    if (found != kShNoSlot) return found;
    const uint32_t base = sh_bucket_base(key, capacity);
    for (uint32_t i = 0; i < kShBucket; i++) {
        uint64_t seen = keys[base + i];
        if (seen == 0u) seen = sh_claim(keys + base + i, key);
        if (seen == 0u || seen == key) return base + i;
    }
    return kShNoSlot;
}

// ---------------------------------------------------------------------------------------------------- voxel
// a component that is NaN or not positive counts 0, one above kShMaxContribution (inf included) counts kShMaxContribution
PT_HD uint32_t sh_quantise(float x)
{
    const float c = !(x > 0.0f) ? 0.0f : (x > kShMaxContribution ? kShMaxContribution : x);
    return (uint32_t)pt_fma(c, kShRadianceScale, 0.5f);
}

PT_HD void sh_add_u32(uint32_t* p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (v) atomicAdd(p, v);
#else
    *p += v;
#endif
}

PT_HD void sh_add(uint4* accum, uint32_t slot, f3 radiance, uint32_t samples)
{
    uint32_t* v = reinterpret_cast<uint32_t*>(accum + slot);
    sh_add_u32(v + 0, sh_quantise(radiance.x));
    sh_add_u32(v + 1, sh_quantise(radiance.y));
    sh_add_u32(v + 2, sh_quantise(radiance.z));
    sh_add_u32(v + 3, samples);
}

PT_HD uint32_t sh_samples(const uint4& v) { return v.w & kShMaxSamples; }
PT_HD uint32_t sh_frames(const uint4& v) { return (v.w >> kShSampleBits) & 0xFFu; }
PT_HD uint32_t sh_stale(const uint4& v) { return v.w >> (kShSampleBits + kShFrameBits); }

// sum / (n kRadianceScale) of a resolved voxel with samples
PT_HD f3 sh_radiance(const uint4& v)
{
    const float d = (float)sh_samples(v) * kShRadianceScale;
    return make_f3((float)v.x / d, (float)v.y / d, (float)v.z / d);
}

// One slot of the resolve (SHARC.hlsl:35-57): this frame's accumulators joined to the previous resolved voxel.  Returns the new
// resolved voxel; clear = the slot's key is to be erased (the voxel returned is zero).
//   sums and samples add (64-bit); frames = previous frames + 1;
//   frames > AccumulationFrames: sums and samples are scaled by AccumulationFrames / frames (integer, rounding down; a voxel with
//   samples keeps at least one), frames = AccumulationFrames;
//   while samples exceed kShMaxSamples or a sum exceeds 32 bits: everything is halved;
//   no sample this frame: stale + 1, and above MaxStaleFrames the slot is cleared; else stale = 0.
PT_HD uint4 sh_resolve_slot(const uint4& acc, const uint4& prev, uint32_t accumulation_frames, uint32_t max_stale_frames, bool& clear)
{
    uint64_t s[3] = { (uint64_t)acc.x + prev.x, (uint64_t)acc.y + prev.y, (uint64_t)acc.z + prev.z };
    uint64_t n = (uint64_t)acc.w + sh_samples(prev);
    uint32_t frames = sh_frames(prev) + 1u;
    uint32_t stale = acc.w ? 0u : sh_stale(prev) + 1u;
    uint4 r;
    r.x = r.y = r.z = r.w = 0u;
    clear = stale > max_stale_frames;
    if (clear) return r;
    if (frames > accumulation_frames) {
        const uint64_t n0 = n;
        for (int k = 0; k < 3; k++) s[k] = s[k] * accumulation_frames / frames;
        n = n * accumulation_frames / frames;
        if (n0 && !n) n = 1u;
        frames = accumulation_frames;
    }
    for (int it = 0; it < 33 && (n > kShMaxSamples || s[0] > 0xFFFFFFFFull || s[1] > 0xFFFFFFFFull || s[2] > 0xFFFFFFFFull); it++) {
        for (int k = 0; k < 3; k++) s[k] >>= 1;
        n >>= 1;
    }
    r.x = (uint32_t)s[0]; r.y = (uint32_t)s[1]; r.z = (uint32_t)s[2];
    r.w = (uint32_t)n | (frames << kShSampleBits) | (stale << (kShSampleBits + kShFrameBits));
    return r;
}

// ---------------------------------------------------------------------------------------------------- anti-firefly filter (spec S25)
// Y(c), left to right, no fma
PT_HD float sh_luminance(f3 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }

// sum / (n kRadianceScale) of this frame's accumulators, whose count is the whole word (sh_radiance masks a resolved voxel's to 16 bits)
PT_HD f3 sh_accum_mean(const uint4& acc)
{
    const float d = (float)acc.w * kShRadianceScale;
    return make_f3((float)acc.x / d, (float)acc.y / d, (float)acc.z / d);
}

// trunc(float(sum) * s) for s in (0, 1], never above sum: float(sum) rounds to nearest and may lie above sum (at 2^32 for the largest
// sums, which no uint32_t holds), and s may have rounded to 1
PT_HD uint32_t sh_ff_scale(uint32_t sum, float s)
{
    const float t = (float)sum * s;
    if (!(t < 4294967296.0f)) return sum;
    const uint32_t r = (uint32_t)t;
    return r < sum ? r : sum;
}

// The resolve's clamp: where the voxel has a history of kShFfMinSamples samples over kShFfMinFrames frames and this frame brought
// samples whose mean luminance Y_a exceeds K max(Y(history), kShFfFloor), the three sums are scaled by K Y_p / Y_a (one division, one
// multiplication per sum, truncation); the count stays.  true = clamped.  Every value is finite: the history has samples, Y_a > 0 where
// it is divided by.
PT_HD bool sh_ff_clamp(uint4& acc, const uint4& prev)
{
    const uint32_t n_p = sh_samples(prev);
    if (!(acc.w > 0u && n_p >= kShFfMinSamples && sh_frames(prev) >= kShFfMinFrames)) return false;
    const float y_p = pt_max(sh_luminance(sh_radiance(prev)), kShFfFloor);
    const float y_a = sh_luminance(sh_accum_mean(acc));
    const float k = kShFfClampBase + kShFfClampSlope / (float)n_p;
    const float limit = k * y_p;
    if (!(y_a > limit)) return false;
    const float s = limit / y_a;
    acc.x = sh_ff_scale(acc.x, s);
    acc.y = sh_ff_scale(acc.y, s);
    acc.z = sh_ff_scale(acc.z, s);
    return true;
}

// sh_resolve_slot with the clamp in front of the join
PT_HD uint4 sh_resolve_slot_ff(const uint4& acc, const uint4& prev, uint32_t accumulation_frames, uint32_t max_stale_frames, bool& clear)
{
    uint4 a = acc;
    (void)sh_ff_clamp(a, prev);
    return sh_resolve_slot(a, prev, accumulation_frames, max_stale_frames, clear);
}

// ---------------------------------------------------------------------------------------------------- update (SHARC_UPDATE)
struct ShState {
    uint32_t slot[kShPropagationDepth - 1u];
    f3 weight[kShPropagationDepth - 1u];
    uint32_t length;   // stored vertices
    bool skipped;      // the last vertex found no slot: its segment's throughput joins the stored one
    uint32_t stopped;  // kFf: walks the weight threshold stopped (a statistic the host-side tests read; the kernels never do)
};

// SharcUpdateMiss, and the tail of SharcUpdateHit: the radiance through the stored weights into every stored vertex, without samples
PT_HD void sh_propagate(const ShMap& m, const ShState& st, f3 radiance)
{
PT_SH_UNROLL
    for (uint32_t i = 0; i < kShPropagationDepth - 1u; i++) {  // (fixed bounds: the state stays in registers)
        if (i < st.length) {
            radiance = radiance * st.weight[i];
            sh_add(m.accum, st.slot[i], radiance, 0u);
        }
    }
}

// sh_propagate with the anti-firefly filter's weight threshold (spec S25): W, the running product of the stored weights, is multiplied
// as the radiance is, and the walk stops in front of the first vertex where Y(W) exceeds kShFfWeightThreshold: that vertex and every
// one behind it receive nothing of this radiance.  (A NaN luminance compares false and stops nothing: sh_quantise counts a NaN as 0.)
PT_HD void sh_propagate_ff(const ShMap& m, ShState& st, f3 radiance)
{
    f3 W = make_f3(1.0f, 1.0f, 1.0f);
    bool open = true;
PT_SH_UNROLL
    for (uint32_t i = 0; i < kShPropagationDepth - 1u; i++) {
        if (i < st.length && open) {
            radiance = radiance * st.weight[i];
            W = W * st.weight[i];
            if (sh_luminance(W) > kShFfWeightThreshold) { open = false; st.stopped++; }
            else sh_add(m.accum, st.slot[i], radiance, 0u);
        }
    }
}

template <bool kFf>
PT_HD void sh_propagate_t(const ShMap& m, ShState& st, f3 radiance)
{
    if constexpr (kFf) sh_propagate_ff(m, st, radiance);
    else sh_propagate(m, st, radiance);
}

// SharcUpdateHit: false = the path ends here (it took the previous frame's radiance of the voxel).  kFf: the radiance goes back
// through sh_propagate_ff; the vertex's own (emission, 1 sample) is added as without the filter.
template <bool kFf>
PT_HD bool sh_update_hit_t(const ShGrid& g, const ShMap& m, ShState& st, f3 P, f3 front_normal, f3 emission, float rnd, uint32_t& failed)
{
    float voxel;
    const uint64_t key = sh_key_at(g, P, front_normal, voxel);
    const uint32_t slot = sh_insert(m.keys, m.capacity, key);
    if (slot == kShNoSlot) {  // the bucket is full: the path goes on without this vertex
        failed++;
        sh_propagate_t<kFf>(m, st, emission);
        st.skipped = true;
        return true;
    }
    bool go_on = true;
    f3 radiance = emission;
    const uint32_t depth = (uint32_t)pt_fma(2.0f, rnd, 1.5f);  // round(lerp(1, kShPropagationDepth - 1, rnd))
    if (depth <= st.length) {
        const uint4 v = m.resolved[slot];
        if (sh_samples(v) > 0u) { radiance = sh_radiance(v); go_on = false; }
    }
    if (go_on) sh_add(m.accum, slot, emission, 1u);
    sh_propagate_t<kFf>(m, st, radiance);
PT_SH_UNROLL
    for (uint32_t i = kShPropagationDepth - 2u; i > 0u; i--) { st.slot[i] = st.slot[i - 1u]; st.weight[i] = st.weight[i - 1u]; }
    st.slot[0] = slot;
    st.weight[0] = make_f3(1.0f, 1.0f, 1.0f);
    st.length = st.length + 1u < kShPropagationDepth - 1u ? st.length + 1u : kShPropagationDepth - 1u;
    st.skipped = false;
    return go_on;
}

PT_HD bool sh_update_hit(const ShGrid& g, const ShMap& m, ShState& st, f3 P, f3 front_normal, f3 emission, float rnd, uint32_t& failed)
{
    return sh_update_hit_t<false>(g, m, st, P, front_normal, emission, rnd, failed);
}

// SharcSetThroughput
PT_HD void sh_set_throughput(ShState& st, f3 T)
{
    if (!st.length) return;
    st.weight[0] = st.skipped ? st.weight[0] * T : T;
}

// clamp(uint(u * n), 0, n - 1) of the update's LOAD (Raytracing.hlsl:69); a product that is NaN or below 1 is texel 0
PT_HD uint32_t sh_texel(float u, uint32_t n)
{
    const float f = u * (float)n;
    return !(f >= 1.0f) ? 0u : (f >= (float)n ? n - 1u : (uint32_t)f);
}

// DI = Diffuse.rgb + Specular.rgb of one texel (one addition per channel, .w is not read); true = any(DI > 0), the reference's isDIValid (:161)
PT_HD bool sh_load_di(const ShFrame& fr, size_t index, f3& DI)
{
    const float4 a = fr.di_diffuse[index], b = fr.di_specular[index];
    DI = load3(a) + load3(b);
    return DI.x > 0.0f || DI.y > 0.0f || DI.z > 0.0f;
}

// One path of the update pass: path (x, y) of the grid fr.cam was made for (InvW, InvH = 1 / grid size).
// kEx (spec S24) with fr.di_diffuse: the first vertex takes the DI of the texel the path's UV falls in, and the second vertex's emission
// is dropped where that DI is valid, unless the path left the first one through the transmission lobe (:302, :311).
// kFf (spec S25): the radiance goes back through sh_propagate_ff.  st: the path's state, the caller's, so that a host-side test can read
// st.stopped afterwards.
template <bool kEx, bool kFf, typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD void sh_update_walk(const ShFrame& fr, const ShGrid& g, const ShMap& m, uint32_t x, uint32_t y, TraceFn&& trace, MaterialFn&& material, EnvFn&& env,
                          ShState& st, uint32_t& rays, uint32_t& failed)
{
    uint32_t rng = rng_init(x, y, fr.frame_index);
    CameraParams cam = fr.cam;
    cam.JitterX = cam.JitterY = rng_float(rng) - 0.5f;  // Raytracing.hlsl:110-116
    f3 o, d;
    float tmin, tmax;
    primary_ray(cam, x, y, o, d, tmin, tmax);
    const bool with_di = kEx && fr.di_diffuse != nullptr;
    uint32_t texel = 0u;
    bool drop_emission = false;  // kEx: the next vertex is the second one and the first one's DI covers its emission
    if (with_di) {  // u, v as primary_ray forms them
        const float u = ((float)x + 0.5f + cam.JitterX) * cam.InvW, v = ((float)y + 0.5f + cam.JitterY) * cam.InvH;
        texel = sh_texel(v, fr.di_h) * fr.di_w + sh_texel(u, fr.di_w);
    }
    st.length = 0u;
    st.skipped = false;
    st.stopped = 0u;
PT_SH_UNROLL
    for (uint32_t i = 0; i < kShPropagationDepth - 1u; i++) { st.slot[i] = 0u; st.weight[i] = make_f3(1.0f, 1.0f, 1.0f); }
    for (uint32_t bounce = 0;; bounce++) {
        float t;
        uint32_t id;
        trace(o, d, tmin, tmax, t, id);
        rays++;
        if (id == 0xFFFFFFFFu) {
            sh_propagate_t<kFf>(m, st, env(d));
            return;
        }
        HitMaterial hm = material(id, o, d, t, bounce == 0u);
        hm.bsdf.Roughness = pt_max(hm.bsdf.Roughness, fr.roughness_threshold);  // :307
        const f3 front_normal = hm.hf.front ? hm.hf.N : -hm.hf.N;
        f3 radiance = hm.emission;
        bool di_valid = false;
        if (with_di && bounce == 0u) {
            f3 DI;
            di_valid = sh_load_di(fr, texel, DI);
            if (di_valid) radiance = DI + radiance;
        }
        if (kEx && bounce == 1u && drop_emission) radiance = make_f3(0.0f, 0.0f, 0.0f);
        if (!sh_update_hit_t<kFf>(g, m, st, hm.hf.P, front_normal, radiance, rng_float(rng), failed)) return;
        if (bounce == fr.bounces) return;
        const Surf surf = surf_init(hm.hf.front, hm.hf.N, hm.Ns);
        const f3 V = -d;
        float w[3];
        lobe_weights(hm.bsdf, surf, V, w);
        float rnd[4];
        rnd[0] = rng_float(rng); rnd[1] = rng_float(rng); rnd[2] = rng_float(rng); rnd[3] = rng_float(rng);
        f3 L;
        int lobe;
        if (!bsdf_sample(hm.bsdf, surf, V, w, rnd, L, lobe)) return;
        if (kEx && bounce == 0u) drop_emission = di_valid && lobe != kLobeTransmission;
        float pdf;
        f3 f;
        if (!bsdf_pdf_eval(hm.bsdf, surf, L, V, w, lobe, pdf, f)) return;
        if (f.x == 0.0f && f.y == 0.0f && f.z == 0.0f) return;
        f3 T = f * pt_rcp(pdf);  // throughput restarts from 1 at every vertex (:215-217)
        if (fr.rr_enabled && bounce > 3u) {
            const float p = pt_max(T.x, pt_max(T.y, T.z));
            if (rng_float(rng) >= p) return;
            T = T * pt_rcp(p);
        }
        sh_set_throughput(st, T);  // no luminance cut-off (:358-360)
        o = spawn_origin(hm.hf.P, hm.hf.N, hm.hf.offset, L);
        d = L;
        tmin = 0.0f; tmax = kInf;
    }
}

template <bool kEx, typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD void sh_update_path_t(const ShFrame& fr, const ShGrid& g, const ShMap& m, uint32_t x, uint32_t y, TraceFn&& trace, MaterialFn&& material, EnvFn&& env,
                            uint32_t& rays, uint32_t& failed)
{
    ShState st;
    sh_update_walk<kEx, false>(fr, g, m, x, y, trace, material, env, st, rays, failed);
}

template <typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD void sh_update_path(const ShFrame& fr, const ShGrid& g, const ShMap& m, uint32_t x, uint32_t y, TraceFn&& trace, MaterialFn&& material, EnvFn&& env,
                          uint32_t& rays, uint32_t& failed)
{
    sh_update_path_t<false>(fr, g, m, x, y, trace, material, env, rays, failed);
}

template <typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD void sh_update_path_ex(const ShFrame& fr, const ShGrid& g, const ShMap& m, uint32_t x, uint32_t y, TraceFn&& trace, MaterialFn&& material, EnvFn&& env,
                             uint32_t& rays, uint32_t& failed)
{
    sh_update_path_t<true>(fr, g, m, x, y, trace, material, env, rays, failed);
}

// sh_update_path_ex with the anti-firefly filter (spec S25); returns the walks the weight threshold stopped
template <typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD uint32_t sh_update_path_ff(const ShFrame& fr, const ShGrid& g, const ShMap& m, uint32_t x, uint32_t y, TraceFn&& trace, MaterialFn&& material, EnvFn&& env,
                                 uint32_t& rays, uint32_t& failed)
{
    ShState st;
    sh_update_walk<true, true>(fr, g, m, x, y, trace, material, env, st, rays, failed);
    return st.stopped;
}

// ---------------------------------------------------------------------------------------------------- query (SHARC_QUERY)
// Raytracing.hlsl:265-274: the hit is far enough for its voxel, and the path has spread wider than the voxel
PT_HD bool sh_valid_hit(float distance, float voxel, float& previous_roughness)
{
    bool valid = distance > voxel * 1.7320508075688772f;
    previous_roughness = pt_min(previous_roughness, 0.99f);
    const float alpha = previous_roughness * previous_roughness;
    const float footprint = distance * pt_sqrt(0.5f * alpha * alpha / (1.0f - alpha * alpha));
    return valid && footprint > voxel;
}

// HashGridDebugColoredHash: a colour of the key's hash
PT_HD f3 sh_debug_colour(uint64_t key)
{
    const uint32_t h = hash32((uint32_t)key ^ hash32((uint32_t)(key >> 32)));
    return make_f3((float)(h & 0xFFu) * (1.0f / 255.0f), (float)((h >> 8) & 0xFFu) * (1.0f / 255.0f), (float)((h >> 16) & 0xFFu) * (1.0f / 255.0f));
}

// One pixel of the frame: pt_render's loop (one primary hit shared by the samples, the RNG running on across them) with the cache
// look-up at every hit; m.keys = null: the cache is off.  With no voxel found the arithmetic is pt_render's, operation for operation.
// kEx (spec S24; what the pixel's finish needs beside the radiance returned): px_flags, hd = sample 0's bounce-1 hit distance (+inf
// without one), prim = the primary hit's emission (the NRD modes only).  In modes 0 / 1 with fr.di_diffuse the sample takes the pixel's
// DI (at out_index) at bounce 0 where it is valid, and drops its bounce-1 emission unless it left through the transmission lobe.
enum : uint32_t {
    kShPxHit = 1u,         // the primary ray hit
    kShPxDiffuse = 2u,     // isDiffuse of spec S13 (sample 0's lobe at bounce 0; true where it spawned no bounce-1 ray)
    kShPxVisualised = 4u,  // the radiance is the hash-grid visualisation's colour
    kShPxDrop = 8u,        // (within a sample) the bounce-1 emission is covered by the DI
};

template <bool kEx, typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD f3 sh_query_pixel_t(const ShFrame& fr, const ShGrid& g, const ShMap& m, uint32_t px, uint32_t py, uint32_t out_index, TraceFn&& trace, MaterialFn&& material,
                          EnvFn&& env, uint32_t& rays, uint32_t& px_flags, float& hd, f3& prim)
{
    f3 o0, d0;
    float tmin, tmax, t0;
    uint32_t id0;
    primary_ray(fr.cam, px, py, o0, d0, tmin, tmax);
    trace(o0, d0, tmin, tmax, t0, id0);
    rays++;
    if (id0 == 0xFFFFFFFFu) return env(d0);
    uint32_t rng = rng_init(px, py, fr.frame_index);
    f3 acc = make_f3(0.0f, 0.0f, 0.0f);
    const bool with_di = kEx && fr.di_diffuse != nullptr && fr.dn_mode < 2u;  // (the NRD modes' query does not read it: :155-158)
    if (kEx) { px_flags = kShPxHit | kShPxDiffuse; hd = kInf; }
    // INVARIANT (kEx): iterations with sample < spp are the samples.  In the NRD modes one more follows with sample == spp, the
    // material-only pass: it fetches the primary hit's material into prim and leaves the bounce loop at once.  Nothing else of the body
    // may run in it -- no RNG draw, no ray, no write of hd or of a flag the finish reads -- and it adds srad = 0 to acc before the pixel returns.
    for (uint32_t sample = 0;;) {
        f3 o = o0, d = d0, T = make_f3(1.0f, 1.0f, 1.0f), srad = make_f3(0.0f, 0.0f, 0.0f);
        float t = t0, previous_roughness = 0.0f;
        uint32_t id = id0;
        if (kEx) px_flags &= ~kShPxDrop;
        for (uint32_t bounce = 0;; bounce++) {
            if (id == 0xFFFFFFFFu) {
                srad = srad + T * env(d);  // :254
                break;
            }
            const HitMaterial hm = material(id, o, d, t, bounce == 0u);
            if (kEx && sample == fr.spp) { prim = hm.emission; break; }  // the finish's pass (below)
            if (m.keys) {
                float voxel;
                const uint64_t key = sh_key_at(g, hm.hf.P, hm.hf.front ? hm.hf.N : -hm.hf.N, voxel);
                if (sh_valid_hit(t, voxel, previous_roughness)) {
                    const uint32_t slot = sh_find(m.keys, m.capacity, key);
                    if (slot != kShNoSlot) {
                        const uint4 v = m.resolved[slot];
                        if (sh_samples(v) > 0u) {
                            if (fr.visualize) {  // :279-284: the primary hit's cell
                                const HitMaterial h0 = material(id0, o0, d0, t0, true);
                                float v0;
                                if (kEx) px_flags |= kShPxVisualised;
                                return sh_debug_colour(sh_key_at(g, h0.hf.P, h0.hf.front ? h0.hf.N : -h0.hf.N, v0));
                            }
                            srad = srad + T * sh_radiance(v);  // :286
                            break;
                        }
                    }
                }
            }
            const bool t_finite = is_finite(T.x) && is_finite(T.y) && is_finite(T.z);
            f3 emission = hm.emission;
            bool di_valid = false;
            if (kEx && bounce == 1u && (px_flags & kShPxDrop)) emission = make_f3(0.0f, 0.0f, 0.0f);  // :302
            if (with_di && bounce == 0u) {
                f3 DI;
                di_valid = sh_load_di(fr, out_index, DI);
                if (di_valid) srad = srad + (DI + T * emission);  // :318, unconditional
            }
            if (!di_valid && (emission.x != 0.0f || emission.y != 0.0f || emission.z != 0.0f || !t_finite)) srad = srad + T * emission;  // :320
            const bool last = bounce == fr.bounces;
            if (last && sample + 1u == fr.spp) break;  // the sample drawn on the final iteration is never used
            const Surf surf = surf_init(hm.hf.front, hm.hf.N, hm.Ns);
            const f3 V = -d;
            float w[3];
            lobe_weights(hm.bsdf, surf, V, w);
            float rnd[4];
            rnd[0] = rng_float(rng); rnd[1] = rng_float(rng); rnd[2] = rng_float(rng); rnd[3] = rng_float(rng);  // :330
            f3 L;
            int lobe;
            if (!bsdf_sample(hm.bsdf, surf, V, w, rnd, L, lobe)) break;
            if (kEx && di_valid && lobe != kLobeTransmission) px_flags |= kShPxDrop;
            float pdf;
            f3 f;
            if (!bsdf_pdf_eval(hm.bsdf, surf, L, V, w, lobe, pdf, f)) break;
            if (f.x == 0.0f && f.y == 0.0f && f.z == 0.0f) break;
            { const float inv_pdf = pt_rcp(pdf); T = T * (f * inv_pdf); }  // :346
            if (fr.rr_enabled && bounce > 3u) {  // :348-356
                const float p = pt_max(T.x, pt_max(T.y, T.z));
                if (rng_float(rng) >= p) break;
                T = T * pt_rcp(p);
            }
            if (luminance(T) <= fr.throughput_threshold) break;  // :361
            if (last) break;
            previous_roughness += lobe == kLobeDiffuse ? 1.0f : hm.bsdf.Roughness;  // :366
            o = spawn_origin(hm.hf.P, hm.hf.N, hm.hf.offset, L);
            d = L;
            trace(o, d, 0.0f, kInf, t, id);
            rays++;
            if (kEx && sample == 0u && bounce == 0u) {  // :235-239, before the cache look-up
                if (lobe != kLobeDiffuse) px_flags &= ~kShPxDiffuse;  // (transmission counts as specular)
                hd = t;  // (a miss returns its tmax: +inf)
            }
        }
        const f3 total = acc + srad;  // :373 (the finish's pass adds 0 to a sum that is finite or not returned)
        // kEx, the NRD modes: prim is re-derived at the finish, not carried through the samples, by one more pass that enters the bounce
        // loop only as far as the primary hit's material -- the loop's own call, not another inlined copy of it (9 VGPRs in the
        // textured instances)
        const bool finish_pass = kEx && fr.dn_mode >= 2u && sample + 1u == fr.spp;
        if (!(kEx && sample == fr.spp)) sample++;
        if (sample == fr.spp && !finish_pass) {
            if (is_finite(total.x) && is_finite(total.y) && is_finite(total.z)) return total * fr.inv_spp;
            return make_f3(0.0f, 0.0f, 0.0f);
        }
        acc = total;
    }
}

template <typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD f3 sh_query_pixel(const ShFrame& fr, const ShGrid& g, const ShMap& m, uint32_t px, uint32_t py, TraceFn&& trace, MaterialFn&& material, EnvFn&& env,
                        uint32_t& rays)
{
    uint32_t px_flags = 0u;
    float hd = 0.0f;
    f3 prim = make_f3(0.0f, 0.0f, 0.0f);
    return sh_query_pixel_t<false>(fr, g, m, px, py, 0u, trace, material, env, rays, px_flags, hd, prim);
}

PT_HD float4 sh_f4(f3 v, float w)
{
    float4 r;  // (member-wise: the host build's float4 is a plain struct)
    r.x = v.x; r.y = v.y; r.z = v.z; r.w = w;
    return r;
}

// One pixel of pt_render_sharc_ex's frame, stored: `out` and the outputs of fr.dn_mode at out_index, as spec S13 writes them with
// res = the query's radiance.  A primary miss and a visualised pixel write only `out`.
template <typename TraceFn, typename MaterialFn, typename EnvFn>
PT_HD void sh_query_pixel_ex(const ShFrame& fr, const ShGrid& g, const ShMap& m, uint32_t px, uint32_t py, uint32_t out_index, TraceFn&& trace, MaterialFn&& material,
                             EnvFn&& env, uint32_t& rays, float4* out)
{
    uint32_t px_flags = 0u;
    float hd = kInf;
    f3 prim = make_f3(0.0f, 0.0f, 0.0f);
    const f3 res = sh_query_pixel_t<true>(fr, g, m, px, py, out_index, trace, material, env, rays, px_flags, hd, prim);
    const bool plain = !(px_flags & kShPxHit) || (px_flags & kShPxVisualised) != 0u;  // a primary miss (res = the environment), a visualised pixel
    const bool diffuse = (px_flags & kShPxDiffuse) != 0u;
    if (plain || fr.dn_mode < 2u) {
        out[out_index] = sh_f4(res, 1.0f);
        if (!plain && fr.dn_mode == 1u && !diffuse && is_finite(hd)) fr.spec_hit_dist[out_index] = hd;
        return;
    }
    const f3 ind = make_f3(pt_max(res.x - prim.x, 0.0f), pt_max(res.y - prim.y, 0.0f), pt_max(res.z - prim.z, 0.0f));
    const f3 zero = make_f3(0.0f, 0.0f, 0.0f);
    const f3 dif = zero + (diffuse ? ind : zero), spe = zero + (diffuse ? zero : ind);  // (S13's sums with direct halves of 0: :403-405)
    fr.dn_diffuse[out_index] = sh_f4(dif, diffuse ? hd : 0.0f);
    fr.dn_specular[out_index] = sh_f4(spe, diffuse ? 0.0f : hd);
    out[out_index] = sh_f4(prim, 1.0f);
}

#if defined(__HIPCC__)
struct SceneView;
struct PixelMap;
// update: one lane per path of pm (the update grid as a frame of its own); query: one lane per pixel of pm into out[out_index];
// counters: [0] rays traced, [1] inserts that found their bucket full
hipError_t launch_sharc_update(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, unsigned long long* counters, uint32_t grid,
                               hipStream_t stream);
// ff: the anti-firefly filter (spec S25), in the resolve and in the _ex update
hipError_t launch_sharc_resolve(const ShMap& m, uint32_t accumulation_frames, uint32_t max_stale_frames, bool ff, hipStream_t stream);
hipError_t launch_sharc_query(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, float4* out, unsigned long long* counters,
                              uint32_t grid, hipStream_t stream);
// pt_render_sharc_ex (spec S24): the instances that read fr's DI (update, query) and write its denoiser outputs (query)
hipError_t launch_sharc_update_ex(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, unsigned long long* counters, uint32_t grid,
                                  bool ff, hipStream_t stream);
hipError_t launch_sharc_query_ex(const SceneView& sv, const PixelMap& pm, const ShFrame& fr, const ShGrid& g, const ShMap& m, float4* out, unsigned long long* counters,
                                 uint32_t grid, hipStream_t stream);
#endif

}  // namespace pt
