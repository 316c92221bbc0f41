// pt_kernels.h -- launch wrappers of the kernel set (pt_kernels.hip), used by the C-ABI implementation.
#pragma once

#include "pt_device.h"
#include "pt_post.h"
#include "pt_gbuffer.h"
#include "pt_region.h"

namespace pt {

constexpr uint32_t kTraverseThreads = 512;  // launch bound; 8 waves share one LDS copy of the BVH
// threads per traverse-type workgroup: 512 when the BVH is staged in LDS (amortises the copy), 256 when it is read
// from global memory (the per-lane stacks are then the only LDS use, and smaller groups keep more waves resident)
inline uint32_t traverse_threads(bool lds_scene) { return lds_scene ? kTraverseThreads : 256u; }
constexpr uint32_t kShadeThreads = 256;
constexpr uint32_t kTailThreads = 256;
constexpr uint32_t kFusedThreads = 512;  // launch bound of the fused trace+shade kernel (launched with 512 or 256 threads)

// dynamic LDS a launch of a kernel that walks the tree needs: the scene copy if lds_scene, plus `depth` stack entries for each of
// `threads` lanes (0: traverse_threads(lds_scene))
uint32_t traverse_lds_bytes_for(uint32_t n_nodes, uint32_t n, uint32_t depth, bool lds_scene, uint32_t threads = 0);

hipError_t launch_primary(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const RayQueue& q, const Scratch& scratch,
                          float4* out, const FrameCounters& fc, uint32_t grid, hipStream_t stream);
// primary beams: per-8x8-block candidate sphere lists for the primary pass (lists: pm.n_slots / 64 records of 16 dwords)
hipError_t launch_beams(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, float slack, uint32_t* lists, uint32_t* regions, hipStream_t stream);
hipError_t launch_traverse(const SceneView& sv, const RayQueue& q, const uint32_t* count_ptr, uint32_t grid, hipStream_t stream);
hipError_t launch_traverse_dyn(const SceneView& sv, const RayQueue& q, const uint32_t* count_ptr, uint32_t* cursor, unsigned long long* totals, uint32_t grid,
                               hipStream_t stream);
hipError_t launch_shade(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const RayQueue& qin, const RayQueue& qout,
                        const Scratch& scratch, float4* out, const uint32_t* count_in, uint32_t* count_out, uint32_t grid, hipStream_t stream);
hipError_t launch_trace(const SceneView& sv, const float* o, const float* d, uint32_t n_rays, float tmin, int use_bvh, float* out_t,
                        uint32_t* out_id, uint2* out_visits, hipStream_t stream);
hipError_t launch_tail(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const RayQueue& qin, const Scratch& scratch, float4* out,
                       const uint32_t* count_ptr, unsigned long long* tail_rays, unsigned long long* totals, uint32_t grid, hipStream_t stream);
hipError_t launch_flush_counters(uint32_t* counts, uint32_t n_counts, unsigned long long* tail, unsigned long long* totals, uint32_t* host_counts,
                                 hipStream_t stream);
hipError_t launch_bounce(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, const RayQueue& qin, const RayQueue& qout,
                         const Scratch& scratch, float4* out, const uint32_t* count_in, uint32_t* count_out, const FrameCounters& fc,
                         bool primary, bool loop, bool inline2, uint32_t threads, uint32_t grid, hipStream_t stream);
hipError_t launch_unpack_tiles(const float4* packed, float4* frame, uint32_t w, uint32_t h, uint32_t ts, uint32_t tiles_x, uint32_t first0,
                               uint32_t run, uint32_t stride, uint32_t n_parts, uint64_t part_stride, bool rgb, hipStream_t stream);
hipError_t launch_pack_rgb(const float4* src, float* dst, uint64_t n, hipStream_t stream);
// bit 31 of the AlphaMode word of every device material := the sphere has texture maps (tex_maps null: none has)
hipError_t launch_material_map_flags(float4* mats, const uint32_t* tex_maps, uint32_t n, hipStream_t stream);
// alpha-tested hits: out[k] = sorted_id[k] | alpha_class[sorted_id[k]] << 30 (the leaf ids of SceneView::sorted_id)
hipError_t launch_leaf_ids(const uint32_t* sorted_id, const uint32_t* alpha_class, uint32_t n, uint32_t* out, hipStream_t stream);

// di_s non-null (row N7, NRD modes): di receives the diffuse half of the estimate and di_s the specular half
hipError_t launch_di(const SceneView& sv, const PixelMap& pm, const FrameParams& fp, float4* di, uint2* primary_hit, unsigned long long* ray_counter, uint32_t grid,
                     hipStream_t stream, float4* di_s = nullptr);
// pt_render_with_di: per slot of pm, di = dd + ds of its pixel (dd, ds indexed like `out`); di_s non-null (NRD modes): di = dd,
// di_s = ds.  .w = 0.
hipError_t launch_di_gather(const PixelMap& pm, const float4* dd, const float4* ds, float4* di, float4* di_s, hipStream_t stream);
hipError_t launch_tonemap(const float4* hdr, uint32_t* out, uint32_t n, const PtToneMapParams& p, hipStream_t stream);
hipError_t launch_accumulate(float4* accum, const float4* rad, uint32_t n, uint32_t frames_accumulated, hipStream_t stream);
// bloom (row N5, pt_bloom.hip): the 9 chain steps and the merge, 10 launches on `stream`.  chain: bloom_chain(width,
// height).texels float4 of scratch; out may equal in.
hipError_t launch_bloom(const float4* in, float4* out, float4* chain, uint32_t width, uint32_t height, float strength, hipStream_t stream);
// G-buffer (row N6, pt_gbuffer.hip): the 13 surface buffers of the pixels of pm (mode 0, a rect), row-major inside the rect; a null
// pointer is a channel not requested (want = the bits of the non-null ones).  One launch on `stream`.
struct GBufferOut {
    float4* Position;
    float2* FlatNormal;
    float2* GeometricNormal;
    float* LinearDepth;
    float* NormalizedDepth;
    f3* MotionVector;
    float4* BaseColorMetalness;
    f3* DiffuseAlbedo;
    f3* SpecularAlbedo;
    float4* NormalRoughness;
    float* IOR;
    float* Transmission;
    f3* Radiance;
};
hipError_t launch_gbuffer(const SceneView& sv, const PixelMap& pm, const GBufferFrame& fr, const GBufferScene& sc, const GBufferOut& out, uint32_t want,
                          uint32_t grid, hipStream_t stream);

}  // namespace pt
