// pt_device.h -- device-side data layout shared by the kernels (pt_kernels.hip) and the C-ABI
// implementation (pt_api.hip).  See DESIGN.md "Data layout in HBM".
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_bsdf.h"
#include "pt_texture.h"
#include "pt_surface.h"
#include "pt_light.h"
#include "pt_pixel_map.h"

namespace pt {

// ---- ray queue: SoA of three float4 streams (48 B per ray) + one 8-B hit stream --------------------
//   q0[i] = { o.x, o.y, o.z, bits(slot) }        slot = path slot (-> pixel, scratch index)
//   q1[i] = { d.x, d.y, d.z, bits(rng state) }
//   q2[i] = { T.r, T.g, T.b, bits(flags) }       flags = bounce | sample << 8 | srad_dirty << 24
//   hit[i] = { bits(t), sphere id (0xFFFFFFFF = miss) }
struct RayQueue {
    float4* q0;
    float4* q1;
    float4* q2;
    uint2* hit;
};

constexpr uint32_t kFlagBounceMask = 0xFFu;
constexpr uint32_t kFlagSampleShift = 8;
constexpr uint32_t kFlagSampleMask = 0xFFFFu;
constexpr uint32_t kFlagDirty = 1u << 24;
constexpr uint32_t kFlagViaTransmission = 1u << 25;  // row N4: this sample left the primary surface through the transmission lobe
constexpr uint32_t kFlagDnSpecular = 1u << 26;       // row N7 (denoiser frames only): sample 0 left the primary surface through a lobe other than diffuse
constexpr uint32_t kMissId = 0xFFFFFFFFu;

// Alpha-tested hits (DESIGN.md spec S10; Scene.ixx:242-243, RaytracingHelpers.hlsli:19-43, ShadingHelpers.hlsli:105-115).  A sphere whose
// AlphaMode is not Opaque is classified on the host when materials or texture maps change:
//   kAlphaVisible    every crossing is accepted: Opaque, or constant alpha (no base-colour map is sampled) >= AlphaCutoff
//   kAlphaInvisible  no crossing is accepted: constant alpha < AlphaCutoff (or NaN) -- the sphere does not exist for rays
//   kAlphaTested     alpha = BaseColor.a * the base-colour map's alpha at the crossing: tested per crossing, near root then far root
// The class rides in the two top bits of the leaf ids the traversal reads (SceneView::sorted_id; sphere ids stay below 2^30), so
// a scene without such spheres pays one compare per successful sphere test and nothing else.
enum : uint32_t { kAlphaVisible = 0u, kAlphaTested = 1u, kAlphaInvisible = 2u };
constexpr uint32_t kIdMask = 0x3FFFFFFFu;
constexpr uint32_t kIdClassShift = 30;

// ---- scene view ------------------------------------------------------------------------------------
// BVH node = 64 B = 4 float4 (PtBvhNode of include/pt_api.h):
//   n0 = lo0.xyz, hi0.x   n1 = hi0.yz, lo1.xy   n2 = lo1.z, hi1.xyz   n3 = child0, child1, parent, pad (ints)
struct SceneView {
    const float4* nodes;        // n_nodes * 4
    const float4* wide;         // 4-wide quantised view of the tree (n_nodes * 4, pt_lbvh_gpu.hip collapse4_kernel) or null; global-memory scenes
    const float4* sph_sorted;   // Morton order {cx,cy,cz,r}
    const uint32_t* sorted_id;  // Morton order -> original sphere id | alpha class << 30 (kIdMask, kIdClassShift)
    const float4* sph;          // original order (shade)
    const float4* mats;         // original order, PtMaterial as 4 float4
    uint32_t n;                 // spheres
    uint32_t n_nodes;           // internal nodes (n - 1; 0 when n == 1)
    uint32_t stack_depth;       // traversal stack entries per lane
    uint32_t descent_cap;       // global-memory scenes: node visits per lane before the wave turns to its sphere tests (0 = unbounded)
    uint32_t lds_scene;         // 1: kernels stage nodes + sph_sorted + sorted_id in LDS
    float slab_tiny;            // what slab_rcp puts in place of a zero direction component: 1e-30, or NaN where the scene's coordinates are too large for it
    float env[4];               // SceneData.EnvironmentLightColor
    // row N1 (textured spheres); null when the scene has no textures
    const TexView* tex;         // texture table
    const uint32_t* tex_maps;   // per sphere: 7 texture indices (TextureMapType order) + 1 "has any" flag
    const float4* rot;          // per sphere: object rotation quaternion (x, y, z, w)
    uint32_t env_tex;           // environment map: index into tex, kNoTexture = EnvironmentLightColor / sky
    uint32_t env_cube;          // 1: tex[env_tex .. env_tex + 5] are the faces of a cube map; 0: tex[env_tex] is a lat-long map
    float env_xf[9];            // upper 3x3 of SceneData.EnvironmentLightTransform, row-major
    // row N4 (sphere-light direct illumination): ids of the emissive spheres, in id order
    const uint32_t* lights;
    uint32_t n_lights;
    // alpha-tested hits: per sphere (original order) its class, or null when every sphere is kAlphaVisible; alpha_tested = some
    // sphere is kAlphaTested (only then do the kernels without a texture variant of their own need their kAlphaTex form)
    const uint32_t* alpha_class;
    uint32_t alpha_tested;
};

// ---- slot -> pixel mapping ---------------------------------------------------------------------------
// PixelMap, block_origin / block_pixel and the per-lane slot_to_pixel: pt_pixel_map.h (shared with the host side and the host-compiled tests)

// a share of a primary-beam list build carried by a primary pass (bounce_kernel): blocks [first_block, first_block + n_blocks) of `lists`,
// for a camera at `centre` (this frame's orientation) with Beam::slack `slack`; n_blocks = 0: none
struct BeamJob {
    uint32_t* lists;
    uint32_t first_block, n_blocks;
    float centre[3];
    float slack;
    float right[3], up[3], forward[3];  // the orientation the lists are made for (CameraParams::Right / Up / Forward)
    float margin_px;                     // make_beam: pixels added on every side of a block's outline
};

struct FrameParams {
    CameraParams cam;
    uint32_t frame_index, bounces, spp, rr_enabled;
    float throughput_threshold;
    float inv_spp;        // 1 / (float)spp
    uint32_t di_enabled;  // IsDIEnabled and the scene has emitters: Scratch::di holds this frame's estimate; kDiExternal: the caller supplied it
    const uint32_t* beam_lists;  // primary beams: one 16-dword record per 64 slots {count, sphere ids}; null = every primary ray traverses
    BeamJob beam_job;
    const uint32_t* refl_lists;  // reflection beams: one kReflRecord-dword region record per 64 slots (pt_region.h); null = every bounce-1 ray traverses
};

// FrameParams::di_enabled of a pt_render_with_di frame: the estimate comes from the caller's buffers (gathered into Scratch::di
// before the first pass), so no pass makes one; the kernels treat it as any non-zero value (DI on), only the host's kernel choice differs
constexpr uint32_t kDiExternal = 2u;

// Per-frame device counters, double buffered by frame parity so that the first kernel of a frame can append to this
// frame's counters while its block 0 folds the PREVIOUS frame's into the running totals and zeroes them for the next.
//   counts[k]  = size of ray queue k of this frame (counts[0] = all slots), appended with one atomicAdd per workgroup
//   tail_rays  = rays spawned inside looping kernels of this frame (they never enter a queue)
//   fold_*     = the other parity's counters (a finished frame)
//   totals[0]  = running sum of secondary rays over folded frames, totals[1] = secondary rays of the last folded frame
struct FrameCounters {
    uint32_t* counts;
    uint32_t* fold_counts;
    uint32_t n_counts;  // counts[0..n_counts] are valid in both arrays; each array is followed by n_counts + 1 work
                        // cursors (cursor k hands out the rays of queue k to the ray-replacement traverse kernel)
    unsigned long long* tail_rays;
    unsigned long long* fold_tail;
    unsigned long long* totals;
    uint32_t* host_counts;  // host-mapped (pinned) copy of the queue sizes of the frame being folded: launch-grid estimates
                            // for later frames reach the host without a copy call; may be null
    // Segmented hand-over from the primary pass to the looping pass (null = dense queue): workgroup b of the primary pass
    // appends its surviving rays to its own segment [b * seg_cap, ...) of the queue, through a counter in LDS -- no barrier
    // and no global atomic per batch -- and leaves the segment's size in seg_counts[b]; the looping pass maps a dense index
    // to (segment, offset) through a prefix sum it builds in LDS.
    uint32_t* seg_counts;
    uint32_t n_segs;        // == grid size of the primary pass, <= kMaxSegs
    uint32_t seg_cap;       // entries per segment
    uint32_t fuse_loop;     // 1: the primary pass finishes its own segment itself (no separate looping pass is launched)
    uint32_t coop_walk;     // 1: the 1-spp looping pass (and the fused form's tail) splits each tree walk over the wave's idle lanes (closest_hit_coop)
    // The primary pass over a view with beam lists (bounce_kernel).  Bits 0-15: how many tiles a workgroup's order table may hold (0: slot
    // order; at most kTileTable); bit 16 (kTileOptSky): a tile with an empty list takes the short path; bit 17 (kTileOptInterleave): draw w of
    // workgroup b is tile b + gridDim.x * w (0: the batch map, eight consecutive tiles per batch of blockDim.x slots)
    uint32_t tile_opts;
};

constexpr uint32_t kTileOptSky = 1u << 16, kTileOptInterleave = 1u << 17;

constexpr uint32_t kTileTable = 256;  // entries of the tile order table: a workgroup's tiles of a 4K 1-spp frame (32 batches of 8 waves)

constexpr uint32_t kMaxSegs = 2048;

constexpr uint32_t kCutSlots = 16;  // entries of the cooperative walk's table of tree cuts (pt_trace.h build_cut)

// Row N7 (DESIGN.md spec S13): the outputs of a denoiser frame (pt_render_denoiser); mode 0 = an ordinary frame, and every other field is
// then unused.  The kernels of such frames are the kDn instances; the None kernels never read this.
//   rec[slot]  = {primary emission (prim), hit distance of sample 0's bounce-1 ray (hd; +inf by default)}: written by the first shading of
//                the primary surface (and .w again by sample 0's bounce-1 hit), read when the pixel finishes
//   di_s[slot] = NRD modes with DI: the specular half of the estimate (Scratch::di then holds the diffuse half)
// diffuse / specular / spec_hit_dist are the caller's buffers, indexed like `out` (row-major inside the rect).
struct DenoiseOut {
    uint32_t mode;  // 1 DLSSRayReconstruction, 2 NRDReBLUR, 3 NRDReLAX
    float4* rec;
    float4* di_s;
    float4* diffuse;
    float4* specular;
    float* spec_hit_dist;
};

// per-slot scratch (only touched when needed, see shade kernel)
struct Scratch {
    float4* sample_rad;   // sampleRadiance of the sample in flight (valid when kFlagDirty)
    float4* radiance;     // sum over finished samples (spp > 1)
    uint2* primary_hit;   // cached primary hit for sample regeneration (spp > 1)
    float4* di;           // row N4: direct illumination of the primary surface {rgb, valid} (IsDIEnabled only)
    // spp > 1, untextured scenes (null otherwise): what the first shading of a pixel's primary surface computes and every later sample
    // of that pixel would compute again -- {N.xyz, spawn offset} {lobe weights, sphere id} {primary direction, -} per slot.  Written by
    // the primary pass, read by the looping pass when it regenerates a sample (L2-resident: a lane re-reads its 48 bytes every few steps).
    float4* primary_cache;
    DenoiseOut dn;  // row N7: denoiser frames only (mode != 0)
};

}  // namespace pt
