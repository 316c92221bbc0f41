/* pt_api.h -- C-ABI of the MI355X-native path-tracing hot path (libpt_hip.so).
 *
 * The reference has no plugin/FFI seam; its operator interface for this path is the
 * pass-object pattern.  Each entry point below names the reference interface
 * it replaces (citations into /root/reference):
 *
 *   pt_create / pt_destroy   Raytracing::Raytracing(CommandList&) + GBufferGeneration ctor: PSO / root
 *                            signature / constant-buffer creation   Source/Raytracing.ixx:61-90, GBufferGeneration.ixx:54-68
 *   pt_set_scene             Scene::Load + Refresh -> InstanceData/ObjectData upload
 *                                                       Source/Scene.ixx:123-219, Source/App.cpp:977-1028
 *   pt_build_accel           Scene::CreateAccelerationStructures (BLAS+TLAS via RTXMU)
 *                                                       Source/Scene.ixx:225-284, RaytracingHelpers.ixx:28-74
 *   pt_set_camera            commandList.Copy(*m_GPUBuffers.Camera, {m_camera})   Source/App.cpp:542-553
 *   pt_set_constants         Raytracing::SetConstants(const GraphicsSettings&)    Source/Raytracing.ixx:92-104
 *   pt_render                GBufferGeneration::Render + Raytracing::Render -> Dispatch / DispatchRays(W,H,1)
 *                                                       Source/GBufferGeneration.ixx:80-117, Raytracing.ixx:106-112,228-249
 *   pt_render_gbuffer        GBufferGeneration::Render with its output textures   Source/GBufferGeneration.ixx:80-117
 *   pt_render_denoiser       Raytracing::Render with GraphicsSettings.Denoiser != None   Shaders/Raytracing.hlsl:377-414, Source/App.cpp:1140-1146
 *   pt_nrd_composition       PostProcessing::NRDComposition::Process (pack and compose around NRD)   Source/NRDComposition.ixx,
 *                            Shaders/NRDComposition.hlsl, driven by App::ProcessNRD  Source/App.cpp:1549-1642
 *   pt_render_with_di        Raytracing::Render with IsDIEnabled = isReSTIRDIEnabled   Source/App.cpp:1262, Shaders/Raytracing.hlsl:150-163
 *   pt_nrd_denoise           NRD::NewFrame / Tag / SetConstants / Denoise (a stand-in for NRD, spec S15)   Source/NRD.ixx:88-140,
 *                            Source/App.cpp:1584-1638
 *   pt_nrd_reblur            the same with nrd::Denoiser::REBLUR_DIFFUSE_SPECULAR's own arithmetic (a recurrent-blur stand-in, spec S32)
 *                            Source/Denoiser.ixx:8, Source/App.cpp:1618-1637
 *   pt_restir_di             RTXDI::SetConstants / Render: the DI passes (a stand-in for RTXDI, spec S16)   Source/App.cpp:1187-1227,
 *                            Shaders/DIInitialSampling.hlsl ... DIFinalShading.hlsl over Shaders/RTXDIAppBridge.hlsli
 *   pt_restir_di_sampled     the same with Power_RIS / ReGIR_RIS local-light presampling (spec S22)                 Source/RTXDI.ixx:209-226
 *   pt_restir_di_ex          ... and with BRDF candidates and the boiling filter (spec S23)                         Source/App.cpp:1092-1101
 *   pt_restir_di_full        ... and with pairwise bias correction and final-visibility reuse (spec S26)            Source/RTXDI.ixx:134
 *   pt_render_sharc          Raytracing::Render(commandList, tlas, SHARC&, SHARCSettings) (a stand-in for SHARC, spec S20)   Source/Raytracing.ixx:114-148
 *   pt_render_sharc_ex       ... with IsDIEnabled and a denoiser, the reference's default frame (spec S24)   Source/App.cpp:1255-1268,
 *                            Shaders/Raytracing.hlsl:150-163, 302-318, 376-414
 *   pt_render_lens           Camera::GenerateThinLensRay in front of the bounce loop (declared, never called by the reference; spec S29)
 *                            Shaders/Camera.hlsli:43-54
 *   pt_render_gbuffer_packed GBufferGeneration::Render into the texture formats App::CreateWindowSizeDependentResources gives them (spec S30)
 *                            Source/App.cpp:431-447
 *   pt_render_from_gbuffer   Raytracing::Render's raygen shader as it runs: the primary surface loaded from those textures, not traced
 *                            (spec S30)   Shaders/Raytracing.hlsl:103-386, Source/App.cpp:1235-1268
 *   pt_upscale               XeSS::SetConstants / Tag / Execute (a stand-in for XeSS / DLSS-SR, spec S17)   Source/XeSS.ixx:46-73,
 *                            Source/App.cpp:1682-1708; pt_upscale_input_size: XeSS::GetInputResolution + the Auto rule, App.cpp:1374-1450
 *   pt_nis_sharpen           Streamline::SetConstants(NISOptions) / Tag / Evaluate(kFeatureNIS) (a stand-in for NIS, spec S18)
 *                            Source/App.cpp:1710-1721, Source/Streamline.ixx:73-74
 *   pt_chromatic_aberration  the Post-Processing setting "Chromatic Aberration" (README.md:59, between NVIDIA Image Scaling and Bloom); the
 *                            reference tree holds no source for it, so the arithmetic is this project's own (spec S31)
 *   pt_frame_gen             App::ProcessDLSSFrameGeneration's tags + Streamline's DLSS-G plugin (a stand-in, spec S19)
 *                            Source/App.cpp:1673-1680, 1460-1525
 *   pt_ray_reconstruction    Streamline::SetConstants(DLSSDOptions) / Tag / Evaluate(kFeatureDLSS_RR) (a stand-in for DLSS-RR, spec S21)
 *                            App::ProcessDLSSRayReconstruction, Source/App.cpp:1654-1671
 *   pt_render_tiles / pt_unpack_tiles / pt_set_partition
 *                            (no reference analogue: single adapter) tile partition for multi-GPU, SURVEY 8e
 *   pt_last_error            ThrowIfFailed -> std::system_error text  Source/ErrorHelpers.ixx:16-32
 *
 * Conventions: plain pointers and sizes, status-code errors (no exceptions cross the boundary),
 * opaque context, caller-owned host memory, callee-owned device memory.  A context is not
 * thread-safe (the reference pass objects are driven from the main thread only, App.cpp:565-644).
 * There is NO CPU fallback: pt_create fails with PT_ERR_NO_DEVICE when no HIP device exists.
 */
#ifndef PT_API_H
#define PT_API_H

#include "pt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtContext PtContext;

typedef enum PtStatus {
    PT_OK = 0,
    PT_ERR_INVALID_ARG = 1,
    PT_ERR_NO_DEVICE = 2,
    PT_ERR_HIP = 3,
    PT_ERR_STATE = 4,       /* call order violated (e.g. render before build_accel) */
    PT_ERR_UNSUPPORTED = 5, /* Denoiser requested, a second texture-coordinate set, ... */
    PT_ERR_OOM = 6
} PtStatus;

typedef struct PtConfig {
    int32_t device;         /* HIP device ordinal */
    uint32_t tile_size;     /* multi-GPU tile edge in pixels, a power of two in [8, 1024]; 0 -> 32 */
    uint64_t stream;        /* hipStream_t to run on (e.g. a torch.cuda.Stream's handle); 0 -> context-owned stream, or the
                               legacy default (null) stream with PT_FLAG_DEFAULT_STREAM */
    uint32_t flags;         /* PT_FLAG_* */
    uint32_t frames_in_flight; /* 0 or 1: one frame at a time; 2..8: that many lanes (see PT_FLAG_TWO_FRAMES_IN_FLIGHT).  3 is the
                                  recommended value: up to three lanes run as streams of the highest priority, whose hardware queues
                                  they share with nothing else unless the process creates highest-priority streams of its own; more
                                  lanes share the default-priority queues with every other stream of the process */
} PtConfig;

enum {
    PT_FLAG_NO_LDS_SCENE = 1u,   /* never stage the BVH into LDS (debug / A-B) */
    PT_FLAG_NO_GRAPH = 2u,       /* reserved, no effect: hipGraph replay of the per-frame launches was measured and rejected
                                    (8.4 us host for a 3-kernel graph vs 10.6 us for three launches, slower end to end) */
    PT_FLAG_HOST_LBVH = 4u,      /* build the LBVH on the host instead of on the GPU (debug / A-B) */
    PT_FLAG_SPLIT_KERNELS = 8u,  /* separate traverse / shade kernels with a hit stream instead of the fused bounce kernel */
    PT_FLAG_FAST_BUILD = 64u,    /* always build the device LBVH (the PREFER_FAST_BUILD analogue).  Default: scenes of up to 4096
                                    spheres get a SAH topology built on the host (PREFER_FAST_TRACE, Source/Scene.ixx:247,283) */
    PT_FLAG_DEFAULT_STREAM = 32u, /* with stream == 0: run on the legacy default stream instead of a context-owned one */
    PT_FLAG_TWO_FRAMES_IN_FLIGHT = 16u /* frames in flight (same as PtConfig.frames_in_flight = 2; that field allows up to 8):
                                          consecutive render calls rotate over N internal streams ("lanes", each with its own
                                          work buffers) so that the latency-bound tail of one frame overlaps the start of the
                                          next ones.  The caller must rotate over N output buffers; whatever it queues on
                                          `stream` after a render call is ordered after that frame.  A frame itself is ordered
                                          after what the caller had queued on `stream` before the render call N - 1 calls
                                          earlier (the consumer of its buffer) -- NOT after work queued since then: do not
                                          clear or fill an output buffer on `stream` right before rendering into it (every
                                          pixel and every padding pixel is written by the frame anyway). */
};

typedef struct PtAccelInfo {
    uint32_t leaf_count;     /* == sphere count */
    uint32_t node_count;     /* internal nodes (leaf_count - 1, or 0 for a single sphere) */
    uint32_t depth;          /* max root-to-leaf edge count */
    uint32_t lds_resident;   /* 1 if traversal stages the whole BVH in LDS */
    float bounds_min[3];
    float bounds_max[3];
    float build_ms;          /* device or host build time */
    uint32_t builder;        /* PT_BUILDER_*: which builder made the topology */
} PtAccelInfo;

enum { PT_BUILDER_DEVICE_LBVH = 0, PT_BUILDER_HOST_LBVH = 1, PT_BUILDER_HOST_SAH = 2 };

typedef struct PtStats {
    uint64_t rays;              /* CastRay-equivalents traced, primaries included */
    uint64_t paths;             /* (pixel, sample) pairs started */
    uint64_t pixels;            /* pixels rendered by this call */
    double ms_total;            /* device time of the whole call (HIP events on the context's stream) */
    double ms_traverse;         /* summed device time of the traverse launches (0 unless profiling on) */
    double ms_shade;            /* summed device time of the shade launches (0 unless profiling on) */
    uint32_t traverse_launches;
    uint32_t shade_launches;
    uint64_t bytes_algorithmic; /* DESIGN.md byte model: per-ray queue traffic + per-path accumulate/store */
    double ms_tail;             /* device time of the fused tail launch (0 unless profiling on) */
    uint32_t tail_launches;
    uint32_t beams_used;        /* pt_render*: 1 = the primary pass took its candidates from primary-beam lists (the exact ones of a resting
                                   view, or the widened ones that follow a camera travelling and turning smoothly -- DESIGN.md "Primary beams");
                                   pt_get_totals: the number of such frames since the last reset */
    uint64_t rays_first_pass_inline; /* pt_get_totals only: secondary rays the primary passes traced in registers (the first
                                        bounce of a 1-spp frame never enters a queue); part of `rays` */
    uint64_t node_visits;       /* pt_get_totals only, scenes traversed in global memory: BVH node records read and ... */
    uint64_t sphere_tests;      /* ... sphere records tested by the traversal kernels (the scene term of the byte accounting) */
} PtStats;

/* BVH node as traversed on the device (DESIGN.md "LBVH layout"); exposed for structural tests. */
typedef struct PtBvhNode {
    float lo0[3], hi0[3];   /* child 0 AABB (padded) */
    float lo1[3], hi1[3];   /* child 1 AABB (padded) */
    int32_t child0, child1; /* >= 0: internal node index; < 0: leaf, Morton-sorted sphere index = ~child */
    int32_t parent;         /* -1 for the root */
    int32_t _pad;
} PtBvhNode;

PtStatus pt_create(const PtConfig *config, PtContext **out_ctx);
void pt_destroy(PtContext *ctx);

/* Copies n spheres + n materials (material i belongs to sphere i == ObjectIndex) and the scene constants.  n == 0 is a legal scene
 * (a TLAS without instances; the pointers may be NULL): every ray misses and every pixel is the environment.
 * Materials whose AlphaMode is not Opaque make their sphere non-opaque geometry, as Scene::CreateAccelerationStructures does
 * (Source/Scene.ixx:242-243): every closest-hit query of the path (primary, bounce and shadow rays, pt_trace_rays) then runs
 * TraceRay's candidate loop for it (Shaders/RaytracingHelpers.hlsli:19-43) -- a crossing of the ray with the sphere's surface counts
 * only if IsOpaque accepts it: BaseColor.a, times the alpha of the base-colour map at that crossing once pt_set_textures has
 * given the sphere one, >= AlphaCutoff; the near crossing is tried first, then the far one (DESIGN.md spec S10). */
PtStatus pt_set_scene(PtContext *ctx, const PtSphere *spheres, const PtMaterial *materials, uint32_t n,
                      const PtSceneData *scene_data);
/* Builds the LBVH over the current spheres.  info may be NULL. */
PtStatus pt_build_accel(PtContext *ctx, PtAccelInfo *info);
/* Moving spheres (the reference rebuilds its TLAS every frame while the physics runs, Source/App.cpp:605-608):
 * pt_update_spheres uploads new centres / radii for the SAME n objects, pt_refit_accel recomputes every box of the
 * existing tree bottom-up (the topology of the last pt_build_accel is kept; any valid BVH gives identical images, only
 * traversal cost drifts -- call pt_set_scene + pt_build_accel again to rebuild).  Both are asynchronous.  The moved spheres hold for
 * every frame from the next render call on, until they are moved again: the lane of the next frame receives them here, the other lanes
 * take them over (and refit) when they render next.  pt_refit_accel may be omitted -- a render call whose lane has not been refitted since
 * the spheres moved refits by itself; calling it lets the refit start before the render call is made. */
PtStatus pt_update_spheres(PtContext *ctx, const PtSphere *spheres, uint32_t n);
PtStatus pt_refit_accel(PtContext *ctx);
PtStatus pt_set_camera(PtContext *ctx, const PtCamera *camera);
/* Raytracing::SetConstants.  Denoiser must be 0 (Denoiser::None) and IsShaderExecutionReorderingEnabled is ignored: the denoiser
 * outputs are requested per frame, by calling pt_render_denoiser with the mode instead of pt_render (a mode held in the constants
 * would change what every later pt_render writes, and those need buffers pt_render does not take).
 * IsDIEnabled = 1 (row N4) adds the sphere-light direct-illumination pass, the build's stand-in for the RTXDI passes
 * whose DI texture Raytracing.hlsl:150-163 reads: one emitter / one cone direction per pixel before the bounce passes,
 * the emission of first-bounce hits reached through a reflective lobe dropped (:302), DI added to the radiance (:381). */
PtStatus pt_set_constants(PtContext *ctx, const PtGraphicsSettings *settings);

/* Render rect (NULL = whole RenderSize) of the frame described by the current constants/camera.
 * out: rect.w*rect.h float4 (r,g,b,1), row-major inside the rect; a HOST pointer if out_is_device == 0
 * (synchronous copy-out), else a DEVICE pointer written on the context's stream (asynchronous).
 * stats may be NULL; requesting stats synchronises the stream. */
PtStatus pt_render(PtContext *ctx, const PtRect *rect, void *out, int out_is_device, PtStats *stats);

/* Multi-GPU tile partition: the RenderSize image is cut into tile_size^2 tiles in row-major
 * tile order; tile t belongs to rank (t % world).  pt_tiles_count returns this rank's tile count for the
 * current RenderSize. */
PtStatus pt_set_partition(PtContext *ctx, uint32_t rank, uint32_t world);
uint32_t pt_tiles_count(PtContext *ctx, uint32_t rank);
/* Render this rank's tiles into a packed DEVICE buffer of pt_tiles_count(rank) * tile_size^2 float4
 * (tile-major, row-major inside a tile; pixels outside the image are zero).  Asynchronous unless stats != NULL. */
PtStatus pt_render_tiles(PtContext *ctx, void *out_device_packed, PtStats *stats);
/* Un-swizzle: given the concatenation [rank 0 tiles | rank 1 tiles | ...] where every rank's block is padded
 * to max_tiles_per_rank tiles (what a gather of equal-sized buffers yields), write the full W*H float4 frame. */
PtStatus pt_unpack_tiles(PtContext *ctx, const void *gathered_device, uint32_t max_tiles_per_rank,
                         void *frame_device);
/* Weighted partition.  xGMI is point-to-point, so the rank that assembles the frame receives every other rank's tiles
 * over one link each while its own tiles cost no transfer: giving it a larger share balances render time against
 * exchange time.  A context owns the tiles t with  first <= t % stride < first + run  (in increasing t; run = 0 owns
 * nothing); pt_set_partition(rank, world) is pt_set_partition_ex(rank, 1, world).  Root weight k over N ranks:
 * stride = N - 1 + k, root (0, k, stride), rank r >= 1 (k - 1 + r, 1, stride).  pt_tiles_count_ex counts a range's tiles
 * for the current RenderSize; pt_render_tiles renders the context's range. */
PtStatus pt_set_partition_ex(PtContext *ctx, uint32_t first, uint32_t run, uint32_t stride);
uint32_t pt_tiles_count_ex(PtContext *ctx, uint32_t first, uint32_t run, uint32_t stride);
/* Un-swizzle n_parts packed buffers laid out part_stride_px float4 apart, part i holding the tiles of the range
 * (first0 + i * run, run, stride).  Pixels of tiles outside these ranges are left untouched, so the frame is assembled
 * by one call for the root's own range and one for the gathered ranges. */
PtStatus pt_unpack_tiles_ex(PtContext *ctx, const void *packed_device, uint64_t part_stride_px, uint32_t n_parts,
                            uint32_t first0, uint32_t run, uint32_t stride, void *frame_device);
/* RGB exchange: every pixel of a frame has alpha 1, so the buffers that cross the links can carry 12 instead of 16 bytes
 * per pixel.  pt_pack_rgb copies n_pixels float4 (packed tiles, any number of frames) to 3 floats per pixel;
 * pt_unpack_tiles_rgb is pt_unpack_tiles_ex for such parts (part_stride_px still counts pixels) and writes alpha = 1. */
PtStatus pt_pack_rgb(PtContext *ctx, const void *src_device, uint64_t n_pixels, void *dst_device);
PtStatus pt_unpack_tiles_rgb(PtContext *ctx, const void *packed_device, uint64_t part_stride_px, uint32_t n_parts,
                             uint32_t first0, uint32_t run, uint32_t stride, void *frame_device);

/* Row N1 -- textured spheres: EvaluateMaterial's texture branches + normal mapping (Shaders/ShadingHelpers.hlsli:53-103,
 * 161-235) over analytic sphere UVs / tangents (csrc/pt_texture.h).  Replaces the texture part of Scene::Load
 * (Source/Scene.ixx:123-180: per-object Textures -> TextureMapInfoArray in ObjectData).  Call after pt_set_scene:
 *   textures[n_textures]   decoded images (copied; converted to linear float4 on upload)
 *   object_textures[n]     one TextureMapInfoArray per sphere (n = the scene's sphere count); Descriptor < n_textures or ~0u;
 *                          NULL = no sphere has maps (the table then only holds the environment map)
 *   rotations              n unit quaternions (x, y, z, w): object -> world rotation of each sphere, NULL = identity
 * n_textures == 0 removes all textures.  Every kernel that shades has a textured variant, selected per launch.
 * The table is also where SceneData.EnvironmentLightTextureDescriptor points (row a18's texture branch,
 * ShadingHelpers.hlsli:13-24: a lat-long map, or the first of the six faces of a cube map; usually PT_TEXTURE_RGBA32_FLOAT);
 * pt_render* fails with PT_ERR_STATE while the scene names an environment texture the table does not hold.
 * pt_update_rotations replaces the quaternions (Earth's spin, the Moon's tidal lock: Source/MyScene.ixx:240-291).  It does no
 * device work and does not wait: the frames in flight keep the rotations they were submitted with, every later render call
 * uploads the new ones into its lane's own copy on its own stream.  A base-colour map on a sphere whose AlphaMode is not
 * Opaque makes its alpha test a per-crossing one (pt_set_scene). */
PtStatus pt_set_textures(PtContext *ctx, const PtTexture *textures, uint32_t n_textures,
                         const PtObjectTextures *object_textures, const float *rotations);
PtStatus pt_update_rotations(PtContext *ctx, const float *rotations, uint32_t n);

/* Row N3 -- display transform and progressive accumulation, on the context's stream (asynchronous).
 * pt_tonemap replaces App::Impl::ToneMap (Source/App.cpp:1731-1757, DirectXTK ToneMapPostProcess): hdr = n_pixels float4
 * (r,g,b,_) -> out = n_pixels packed uint32: R8G8B8A8_UNORM for the Linear / SRGB transfer functions, R10G10B10A2_UNORM
 * for ST2084.  Both pointers are DEVICE pointers.
 * pt_accumulate keeps the running mean of successive frames (progressive refinement while the camera rests; the
 * reference accumulates inside its denoisers, which are out of scope): accum = frames_accumulated == 0 ? radiance
 * : accum + (radiance - accum) / (frames_accumulated + 1), per channel, alpha included. */
PtStatus pt_tonemap(PtContext *ctx, const void *hdr_device, uint32_t n_pixels, const PtToneMapParams *params,
                    void *out_device);
PtStatus pt_accumulate(PtContext *ctx, void *accum_device, const void *radiance_device, uint32_t n_pixels,
                       uint32_t frames_accumulated);

/* Row N5 -- bloom (Source/Bloom.ixx, Shaders/Bloom.hlsl, Shaders/Merge.hlsl), on the context's stream (asynchronous).
 * hdr / out = width*height float4, row-major, DEVICE pointers; out == hdr is allowed.  RGB is bloomed, alpha copied:
 * out = hdr * (1 - strength) + blur * strength.  width and height must be >= 32 and strength in [0, 1] (NaN rejected).
 * The context holds the blur chain; a call that needs a larger one than it has waits for the context's stream (the
 * previous bloom calls) before it frees the old chain.  The render lanes' frames in flight never touch it. */
PtStatus pt_bloom(PtContext *ctx, const void *hdr_device, void *out_device, uint32_t width, uint32_t height, float strength);

/* Row N6 -- the G-buffer pass (Source/GBufferGeneration.ixx, Shaders/GBufferGeneration.hlsl; DESIGN.md spec S12): the 13 per-pixel
 * surface buffers of the frame the next pt_render renders (current camera, constants, scene data and textures), for a host's
 * denoiser, upscaler or TAA.  All float32, row-major inside the rect, with the reference's channel counts:
 *   Position float4 (P, PositionOffset) | FlatNormal, GeometricNormal float2 (signed octahedral) | LinearDepth float |
 *   NormalizedDepth float | MotionVector float3 (pixels, pixels, view depth) | BaseColorMetalness float4 | DiffuseAlbedo,
 *   SpecularAlbedo float3 | NormalRoughness float4 | IOR float | Transmission float | Radiance float3 (emission, or the
 *   environment on a miss).
 * A miss writes Position = inf, LinearDepth = inf, NormalizedDepth = IsNormalizedDepthReversed ? 0 : 1, MotionVector and Radiance,
 * and leaves the other buffers untouched; Transmission is written only where Metallic < 1.  Camera.Matrices must be filled
 * (WorldToProjection, and PreviousWorldToProjection / PreviousWorldToView for the motion vectors).
 * Runs asynchronously on the lane of the next pt_render and is ordered like that frame: with frames in flight the caller rotates over
 * as many sets of G-buffer buffers as there are lanes (PT_FLAG_TWO_FRAMES_IN_FLIGHT's contract for frame buffers), and the pass waits
 * for what the caller had queued before the render call N - 1 calls earlier -- or for everything queued so far, before the first render
 * call or when a buffer is one another lane wrote within that window.  What is queued on the context's stream afterwards sees the result.
 * It adds nothing to pt_get_totals and does not advance the frame lanes. */
typedef struct PtGBuffer {          /* DEVICE pointers, NULL = not requested; float4 buffers 16-byte aligned, float2 8-byte */
    void *Position, *FlatNormal, *GeometricNormal, *LinearDepth, *NormalizedDepth, *MotionVector,
         *BaseColorMetalness, *DiffuseAlbedo, *SpecularAlbedo, *NormalRoughness, *IOR, *Transmission, *Radiance;
} PtGBuffer;
/* rect: NULL = the whole RenderSize (UVs are relative to the whole RenderSize either way).  previous_spheres (n PtSphere) and
 * previous_rotations (n quaternions x, y, z, w): host arrays of the scene's n spheres, the previous pose (PreviousObjectToWorld of
 * Scene::Refresh) the motion vectors of hits are measured from; NULL = the same as the current pose; both ignored while
 * SceneData.IsStatic != 0.  PT_ERR_INVALID_ARG: no buffer requested, a misaligned buffer, a bad rect, a previous sphere that is
 * not finite or has radius <= 0, a rotation that is not finite.  PT_ERR_STATE: as pt_render. */
PtStatus pt_render_gbuffer(PtContext *ctx, const PtRect *rect, const PtGBuffer *out,
                           const PtSphere *previous_spheres, const float *previous_rotations);

/* Row N7 -- the bounce loop's denoiser outputs (DESIGN.md spec S13; Raytracing.hlsl:377-414).  An ordinary frame in every respect (the
 * contract of pt_render: lanes, frames in flight, totals, beam lists, refit, textures, alpha) that writes, per pixel of the rect:
 *   Denoiser 1 (DLSSRayReconstruction): out = the radiance pt_render writes; SpecularHitDistance (float) = the hit distance of sample 0's
 *     first bounce where the primary ray hit, that bounce left through a lobe other than diffuse and its ray hit something; else untouched.
 *   Denoiser 2 (NRDReBLUR), 3 (NRDReLAX): out = the primary surface's emission (the environment on a miss); on hits, Diffuse (float4) =
 *     (DI_diffuse + (diffuse ? indirect : 0), diffuse ? hit distance : 0) and Specular (float4) = (DI_specular + (diffuse ? 0 : indirect),
 *     diffuse ? 0 : hit distance), indirect = max(radiance without DI - emission, 0); misses leave both untouched.
 * "diffuse" is the lobe sample 0 took at the primary surface (true when sample 0 ended there; the hit distance is then +inf).  The caller
 * clears the buffers first, as the reference's host does.  Buffers are rect.w * rect.h, row-major inside the rect; with frames in flight
 * the caller rotates one set per lane, as for out, and as for out the rule is enforced: a frame whose buffer (out or a denoiser
 * buffer) is one another lane's frame wrote within that window waits for everything queued before it (correct, at the cost of overlap).  PT_ERR_INVALID_ARG: an unknown mode (0 included), a required buffer missing or
 * misaligned, a bad rect.  PT_ERR_STATE: as pt_render.  The tile entry points render Denoiser::None only. */
typedef struct PtDenoiserOutputs {   /* DEVICE pointers, float4 ones 16-byte aligned */
    uint32_t Denoiser;               /* 1 DLSSRayReconstruction, 2 NRDReBLUR, 3 NRDReLAX (Source/Denoiser.ixx) */
    uint32_t _pad;
    void *Diffuse, *Specular;        /* NRD modes: both required */
    void *SpecularHitDistance;       /* DLSS-RR: required */
} PtDenoiserOutputs;
PtStatus pt_render_denoiser(PtContext *ctx, const PtRect *rect, void *out, int out_is_device,
                            const PtDenoiserOutputs *outputs, PtStats *stats);

/* A frame whose direct illumination the caller supplies: the reference's frame with IsDIEnabled = isReSTIRDIEnabled
 * (Source/App.cpp:1262), whose DI the RTXDI passes make (pt_restir_di below is this library's such pass; any other source of the two buffers serves as well).  In every other respect an ordinary frame under the contract of
 * pt_render (outputs == NULL: Denoiser::None) or of pt_render_denoiser (outputs: its mode and buffers), whatever
 * PtGraphicsSettings.IsDIEnabled says.  Only the source of DI changes: per pixel of the rect, DI = Diffuse.rgb + Specular.rgb
 * (Raytracing.hlsl:160; .w is not read), in place of row N4's estimate, with N4's two gates kept: DI is added only where the primary ray
 * hit, and the emission a first bounce reaches through the transmission lobe is kept (elsewhere it is dropped, as DI covers it).  The
 * NRD modes take the two halves apart (Diffuse into the diffuse output, Specular into the specular one).
 * The buffers are read before the frame's first pass, so they may be the frame's own denoiser outputs (the reference uses them in place
 * that way).  Written on another stream, they must be complete before the call; the frame waits for everything queued on the
 * context's stream before it (with frames in flight: at the cost of their overlap).  They are held to the rotation rule of pt_render's
 * buffers as inputs: a later frame in flight whose out or denoiser buffer is one of them waits until this frame has read them.  The
 * tile entry points render without supplied DI.
 * PT_ERR_INVALID_ARG: a null DI buffer, one not 16-byte aligned, and whatever pt_render / pt_render_denoiser reject. */
typedef struct PtDirectLighting {   /* DEVICE pointers, float4 per pixel of the rect (row-major inside it), 16-byte aligned */
    const void *Diffuse, *Specular; /* the textures DIFinalShading writes (DIFinalShading.hlsl:95-104) */
} PtDirectLighting;
PtStatus pt_render_with_di(PtContext *ctx, const PtRect *rect, void *out, int out_is_device, const PtDirectLighting *di,
                           const PtDenoiserOutputs *outputs, PtStats *stats);

/* Row N8 -- the NRD composition pass (PostProcessing::NRDComposition, Shaders/NRDComposition.hlsl; DESIGN.md spec S14), on the
 * context's stream (asynchronous): ordered after the G-buffer and the denoiser frames already queued, before whatever the caller
 * queues there next; it adds nothing to pt_get_totals.  One pass over the RenderSize[0] x RenderSize[1] pixels (row-major, the
 * rect of the pt_render_gbuffer / pt_render_denoiser calls that made the inputs); a pixel whose LinearDepth is not finite (a miss)
 * is left untouched.
 *   Pack != 0 (before NRD): NoisyDiffuse / NoisySpecular in place: rgb /= the lobe's albedo, then the NRD front-end of the mode
 *     (ReBLUR: hit distance normalised by ReBLURHitDistance and NormalRoughness.w, rgb to YCoCg; ReLAX: sanitised).
 *   Pack == 0 (after NRD): Radiance.rgb += unpack(DenoisedDiffuse).rgb * DiffuseAlbedo + unpack(DenoisedSpecular).rgb * SpecularAlbedo;
 *     alpha unchanged.  In the NRD modes pt_render_denoiser's out holds the primary emission, the radiance this adds to.
 * PT_ERR_INVALID_ARG: a null argument; Denoiser not 2 or 3; a RenderSize of 0 or > 16384; a buffer the direction needs missing
 * (LinearDepth, both albedos, and: pack both noisy buffers, plus NormalRoughness for ReBLUR; compose both denoised buffers and
 * Radiance); a float4 buffer not 16-byte aligned or a float / float3 one not 4-byte aligned; a buffer the call writes overlapping
 * another buffer it uses (Radiance aliasing an input; the two noisy buffers, or one of them and an input). */
typedef struct PtNrdCompositionTextures {   /* DEVICE pointers (NRDComposition::Textures); NULL where the direction does not use it */
    const void *LinearDepth;                /* float   (G-buffer LinearDepth) */
    const void *DiffuseAlbedo;              /* float3  (G-buffer DiffuseAlbedo) */
    const void *SpecularAlbedo;             /* float3  (G-buffer SpecularAlbedo) */
    const void *NormalRoughness;            /* float4  (G-buffer NormalRoughness; ReBLUR pack reads .w) */
    void *NoisyDiffuse, *NoisySpecular;     /* float4  (pt_render_denoiser Diffuse / Specular): pack */
    const void *DenoisedDiffuse;            /* float4  (NRD's OUT_DIFF_RADIANCE_HITDIST): compose */
    const void *DenoisedSpecular;           /* float4  (NRD's OUT_SPEC_RADIANCE_HITDIST): compose */
    void *Radiance;                         /* float4  (pt_render_denoiser out): compose */
} PtNrdCompositionTextures;
PtStatus pt_nrd_composition(PtContext *ctx, const PtNrdCompositionConstants *constants, const PtNrdCompositionTextures *textures);

/* Row N9 -- the NRD stand-in (NRD::Denoise as App::ProcessNRD drives it, Source/NRD.ixx:88-140, Source/App.cpp:1584-1638; DESIGN.md
 * spec S15): a ReLAX-style denoiser of the SVGF family -- temporal accumulation reprojected with the motion vectors, a variance
 * estimate from luminance moments, an edge-stopping a-trous filter -- from the packed In buffers to the Out buffers compose reads.
 * On the context's stream (asynchronous), ordered like pt_nrd_composition: after the G-buffer and denoiser frames already queued,
 * before whatever the caller queues there next; it adds nothing to pt_get_totals.  A pixel whose ViewZ is not finite (a miss) is
 * never written.  The context owns the history (accumulated signal, moments and length per lobe, previous depth and normal),
 * allocated on first use and freed by pt_destroy; the first call, and a call whose RenderSize or Denoiser differs from the previous
 * one, acts as CLEAR_AND_RESTART.
 * PT_ERR_INVALID_ARG: a null argument; Denoiser not 2 or 3; AccumulationMode above 2; a RenderSize of 0 or > 16384; AtrousIterations
 * above 8; a required buffer missing (all but BaseColorMetalness); a float4 buffer not 16-byte aligned or a float / float3 one not
 * 4-byte aligned; an output overlapping an input or the other output. */
typedef struct PtNrdDenoiseTextures {   /* DEVICE pointers; the reference's nrd::ResourceType tags */
    const void *ViewZ;                  /* IN_VIEWZ: G-buffer LinearDepth, float */
    const void *MotionVector;           /* IN_MV: G-buffer MotionVector, float3 (previous - current, pixels; .z linear depth) */
    const void *NormalRoughness;        /* IN_NORMAL_ROUGHNESS: float4 */
    const void *BaseColorMetalness;     /* IN_BASECOLOR_METALNESS: float4, may be NULL (accepted, not read by S15) */
    const void *InDiffuse, *InSpecular; /* IN_DIFF / IN_SPEC_RADIANCE_HITDIST: float4, packed by pt_nrd_composition */
    void *OutDiffuse, *OutSpecular;     /* OUT_DIFF / OUT_SPEC_RADIANCE_HITDIST: float4, what compose reads */
} PtNrdDenoiseTextures;
PtStatus pt_nrd_denoise(PtContext *ctx, const PtNrdDenoiseSettings *settings, const PtNrdDenoiseTextures *textures);

/* Row N30 -- the ReBLUR stand-in (the ReBLUR branch of App::ProcessNRD, Source/App.cpp:1618-1637; DESIGN.md spec S32): a recurrent-blur
 * denoiser of ReBLUR's family -- temporal accumulation into a slow and a fast history (a resting mirror accumulates too), a history fix
 * and a clamp of the slow history to the fast one, then a blur and a post-blur over a rotated 8-point disc whose radius shrinks with the
 * history length and grows with the normalised hit distance; the post-blur's result is Out and the next call's history.  No variance,
 * no luminance edge-stopping.  It takes PtNrdDenoiseTextures unchanged; In and Out are always in ReBLUR's encoding (YCoCg + normalised
 * hit distance: what pt_nrd_composition packs and composes with Denoiser = 2); Out.w is the reconstructed hit distance.  pt_nrd_denoise
 * is unchanged, and the two may alternate on one context: each owns its history (this one: allocated on first use, freed by pt_destroy).
 * On the context's stream (asynchronous), ordered like pt_nrd_denoise; it adds nothing to pt_get_totals.  A pixel whose ViewZ is not
 * finite (a miss) is never written.  The first call, a non-zero AccumulationMode and a change of RenderSize restart the history.
 * The arithmetic is this project's own.  Out of scope: NRD's exact ReBLUR, its pre-pass, temporal stabilisation, virtual-motion specular
 * reprojection, OUT_VALIDATION, and the checkerboard and half-resolution modes.
 * PT_ERR_INVALID_ARG: a null argument; AccumulationMode above 2; a RenderSize of 0 or > 16384; MaxFastAccumulatedFrames above
 * MaxAccumulatedFrames (after the defaults); a radius that is not finite or negative, MinBlurRadius above MaxBlurRadius or MaxBlurRadius
 * above 64 (after the defaults); non-zero padding; and pt_nrd_denoise's buffer rules. */
PtStatus pt_nrd_reblur(PtContext *ctx, const PtNrdReblurSettings *settings, const PtNrdDenoiseTextures *textures);
/* Test / tooling hook: the history slot the last pt_nrd_reblur call wrote, to HOST arrays of RenderSize float4 texels (any may be
 * NULL): the slow history per lobe (the blurred signal, its hit distance: Out itself), the fast history per lobe (the signal, the
 * history length) and the guide (ViewZ, normal).  Waits for the context's stream.  PT_ERR_STATE: no call has been made yet. */
PtStatus pt_nrd_reblur_history(PtContext *ctx, void *slow_diffuse, void *slow_specular, void *fast_diffuse, void *fast_specular, void *guide);

/* Row N10 -- the reservoir pass that makes the DI pt_render_with_di takes (RTXDI::Render, Source/App.cpp:1187-1227; DESIGN.md spec S16): a
 * ReSTIR-DI stand-in for the RTXDI SDK, which the reference does not vendor -- RIS over InitialSamples uniform (emitter, cone) candidates
 * with one visibility ray, temporal reuse of the reprojected pixel's reservoir, spatial reuse of SpatialSamples neighbours, final shading
 * with a visibility ray -- from the G-buffer of the frame the next render call renders (current camera and scene; Camera.PreviousPosition
 * for the history's view vectors) to the two buffers of PtDirectLighting / PtDenoiserOutputs: Diffuse = (Le f_d W / pdf, light distance),
 * Specular likewise with f_s.  A pixel without a surface (LinearDepth not finite, or roughness < 0.05: RTXDIAppBridge.hlsli:295), without
 * a valid reservoir, or whose sum is zero or not finite is not written: the caller clears the buffers, as the reference's host does.
 * With no emitters in the scene the call succeeds and writes nothing.
 * All buffers are DEVICE pointers, float32, row-major over RenderSize (the whole frame: the rect of the pt_render_gbuffer call that made
 * the inputs).  Runs asynchronously on the lane of the next render call and is ordered like pt_render_gbuffer (the same rotation rule for
 * buffers; an input that the lane's own pt_render_gbuffer call did not write makes the pass wait for everything queued on the context's
 * stream); the context's stream waits for the pass.  It adds nothing to pt_get_totals and does not advance the frame lanes.
 * The context owns the history -- two alternating slots of a 68-byte surface record and a 32-byte reservoir per pixel -- allocated on
 * first use and freed by pt_destroy.  The history restarts on the first call, with ResetHistory, when RenderSize changes and after
 * pt_set_scene (emitter indices change); spheres moved by pt_update_spheres keep it.
 * The candidates are uniform over the emitter list; pt_restir_di_sampled below draws them from presampled structures (row N16).
 * BRDF candidates and the boiling filter: pt_restir_di_ex below (row N17).  Pairwise bias correction and final-visibility reuse:
 * pt_restir_di_full below (row N22).
 * Not built (spec S16): environment candidates (the reference's bridge stubs them to 0), checkerboard rendering,
 * the DLSS-RR SpecularHitDistance write.
 * PT_ERR_INVALID_ARG: a null argument; a missing buffer; a float4 buffer not 16-byte aligned, GeometricNormal not 8-byte, another not
 * 4-byte; an output overlapping an input or the other output; a value outside the ranges of PtRestirDiSettings.  PT_ERR_UNSUPPORTED:
 * bias correction mode 2 (Pairwise), which only pt_restir_di_full accepts.  PT_ERR_STATE: as pt_render (the pass casts rays). */
typedef struct PtRestirDiTextures {     /* DEVICE pointers; inputs are what RAB_GetGBufferSurface reads, as pt_render_gbuffer writes them */
    const void *Position;               /* float4 (P, PositionOffset) */
    const void *GeometricNormal;        /* float2 */
    const void *LinearDepth;            /* float */
    const void *MotionVector;           /* float3 */
    const void *BaseColorMetalness;     /* float4 */
    const void *NormalRoughness;        /* float4 */
    const void *IOR;                    /* float */
    const void *Transmission;           /* float (read only where metalness < 1) */
    void *Diffuse, *Specular;           /* float4: outputs */
} PtRestirDiTextures;
PtStatus pt_restir_di(PtContext *ctx, const PtRestirDiSettings *settings, const PtRestirDiTextures *textures);

/* Row N16 -- pt_restir_di with the reference's three local-light sampling modes (ReSTIRDI_LocalLightSamplingMode; DESIGN.md spec S22): a
 * stand-in for the passes the reference runs in front of the DI passes (LightPreparation.hlsl, MipmapGeneration.hlsl,
 * LocalLightPresampling.hlsl, ReGIRPresampling.hlsl; RTXDI::Render, Source/RTXDI.ixx:209-226).  Before launch 1 the call rebuilds, from the
 * spheres the lane's frame sees (pt_update_spheres included), a power pyramid over the emitter list, a Power_RIS tile buffer
 * (TileCount x TileSize entries) and, in ReGIR_RIS mode, a grid of ReGIRGridSize^3 cells of ReGIRCellSize around Camera.Position with
 * ReGIRLightsPerCell entries each; launch 1 then draws its InitialSamples candidates from the pixel block's tile (Power_RIS) or from the
 * cell of the jittered surface point (ReGIR_RIS; outside the grid: the tile).  Everything after initial sampling is pt_restir_di's.
 * `sampling` NULL or Mode 0 (Uniform): the call IS pt_restir_di -- the same history slots, restart rules and bits; calls of the two
 * entry points may alternate on one context and share the history.  Errors, lane, ordering, buffer rotation, profiling slots (plus
 * the presampling launches, as one interval, under ms_tail) and the "no emitters: success, nothing written" rule: as pt_restir_di.
 * Not built: ReGIR's onion mode, the cell visualisation, environment candidates, the compact-light-info path.
 * PT_ERR_INVALID_ARG also: a Mode above 2, a size above its range, a cell size that is not finite or outside [0.1, 10], a nonzero _pad,
 * more than 2^24 entries in the two segments together. */
PtStatus pt_restir_di_sampled(PtContext *ctx, const PtRestirDiSettings *settings, const PtLightSamplingSettings *sampling, const PtRestirDiTextures *textures);

/* Row N17 -- pt_restir_di_sampled with the two remaining defaults of the reference's ReSTIRDI settings block (DESIGN.md spec S23): BrdfSamples
 * BSDF-sampled candidates mixed into initial sampling by the balance heuristic (InitialSampling.BRDFSamples; App.cpp:1092-1095 with
 * brdfCutoff = 0; the callbacks of RTXDIAppBridge.hlsli:394-402, 468-501) -- each costs launch 1 one closest-hit ray -- and the boiling
 * filter over launch 1's temporal result (TemporalResampling.BoilingFilter; DITemporalResampling.hlsl:41-46), per 8x8 pixel block.
 * `candidates` NULL, or BrdfSamples 0 and the filter off: the call IS pt_restir_di_sampled -- the same history slots, restart rules and
 * bits; calls of the three entry points may alternate on one context.  Errors, lane, ordering, buffer rotation, profiling slots: as
 * pt_restir_di_sampled.  The arithmetic is this library's own (the RTXDI SDK is not vendored): no parity with the SDK is claimed.
 * PT_ERR_INVALID_ARG also: BrdfSamples above 8, EnableBoilingFilter above 1, with the filter enabled a strength that is not finite or
 * outside [0, 1], a nonzero _pad. */
PtStatus pt_restir_di_ex(PtContext *ctx, const PtRestirDiSettings *settings, const PtLightSamplingSettings *sampling, const PtRestirDiCandidates *candidates,
                         const PtRestirDiTextures *textures);

/* Row N22 -- pt_restir_di_ex with the two remaining values of the reference's ReSTIRDI settings block (DESIGN.md spec S26):
 *   bias correction mode 2 (Pairwise) in TemporalBiasCorrection and / or SpatialBiasCorrection: pairwise MIS between the centre reservoir
 *     and each accepted neighbour, targets without visibility (among occluders biased the way Basic is; Raytraced stays the unbiased mode);
 *   final-visibility reuse (`shading`): a reservoir's eighth word records that the visibility ray of the surface that drew the sample
 *     reached its emitter, and the pixel offset the sample has travelled since; a sample at most FinalVisibilityMaxAge frames old and
 *     FinalVisibilityMaxDistance pixels away, on an emitter that is not alpha-tested, casts no final ray.  Reuse never changes a reservoir:
 *     a pixel written without it holds the same bits with it; the extra pixels it writes are those an out-of-date visibility lets through.
 *     With both limits 0 the output equals reuse off bit for bit.
 * `shading` NULL or ReuseFinalVisibility 0, and no bias mode equal to 2: the call IS pt_restir_di_ex -- the same launches, history slots,
 * restart rules and bits; calls of the four entry points may alternate on one context (the other three write the word as 0: nothing known).
 * Errors, lane, ordering, buffer rotation, profiling slots: as pt_restir_di_ex.  The arithmetic is this library's own, written from the
 * reference's shaders and from recollection of RTXDI (the SDK is not vendored): no parity with the SDK is claimed.
 * Not built: writing the final ray's result back into the history, discardInvisibleSamples, a ray-traced pairwise variant, checkerboard
 * rendering, environment candidates, ReGIR's onion mode and cell visualisation.
 * PT_ERR_INVALID_ARG also: ReuseFinalVisibility above 1, FinalVisibilityMaxAge above 255, a FinalVisibilityMaxDistance that is not finite
 * or is negative, a nonzero _pad. */
PtStatus pt_restir_di_full(PtContext *ctx, const PtRestirDiSettings *settings, const PtLightSamplingSettings *sampling, const PtRestirDiCandidates *candidates,
                           const PtRestirDiShading *shading, const PtRestirDiTextures *textures);

/* Test hook: a slot of the history pt_restir_di / pt_restir_di_sampled / pt_restir_di_ex / pt_restir_di_full keep, after waiting for the last call: which = 0 the slot the
 * last call wrote, 1 the slot the call before it wrote.  planes: six planes of RenderSize float4 (the surface record's four, then the
 * reservoir's two: {emitter bits, u1, u2, W}, {M, p_hat, age bits, visibility word: 0 = nothing known, all that the first three entry
 * points write; spec S26}); transmission: RenderSize floats.  A pixel without a surface
 * holds only plane 3 (its depth is +inf); its other words are whatever the slot held before.  PT_ERR_STATE: no call has left a history. */
PtStatus pt_restir_di_history(PtContext *ctx, uint32_t which, void *planes, void *transmission);

/* Test hook: what the last pt_restir_di_sampled call with a presampling mode built, after waiting for it.  On entry *n_pyramid and
 * *n_entries hold the capacities of `pyramid` (floats) and `ris` (entries of two uint32: emitter index or 0xFFFFFFFF, bits of
 * 1 / source pdf); on return the counts.  pyramid: every level, leaves first (4^Lv, ..., 4, 1 floats, each level in Z-curve order);
 * ris: the Power_RIS segment, then the ReGIR segment (ReGIR_RIS mode only).  A null array is not filled (its count still is).
 * PT_ERR_STATE: no such call has been made; PT_ERR_INVALID_ARG: a null count or a capacity below the count. */
PtStatus pt_light_ris_download(PtContext *ctx, float *pyramid, uint32_t *n_pyramid, uint32_t *ris, uint32_t *n_entries);

/* Row N14 -- the frame through the radiance cache (Raytracing::Render(commandList, tlas, SHARC&, SHARCSettings), Source/Raytracing.ixx:114-148;
 * DESIGN.md spec S20): a stand-in for the SHARC library, which the reference does not vendor.  Three stages on the lane of the next render
 * call, in this order:
 *   UPDATE   the accumulators are cleared; (W / DownscaleFactor) x (H / DownscaleFactor) paths (the SHARC_UPDATE permutation of
 *            Shaders/Raytracing.hlsl) insert their vertices into the hash grid and add their radiance to them and to the vertices before;
 *   RESOLVE  every voxel joins this frame's sums to its history (Shaders/SHARC.hlsl:35-57), ages, and is evicted when stale;
 *   QUERY    the frame of pt_render (the SHARC_QUERY permutation): a path that meets a voxel with samples, far and wide enough, ends there
 *            with the voxel's radiance.  With an empty cache the frame is pt_render's, bit for bit.
 * Frame settings (RenderSize, FrameIndex, Bounces, SamplesPerPixel, Russian roulette, ThroughputThreshold) come from pt_set_constants;
 * IsDIEnabled and Denoiser must be 0.  rect / out / out_is_device / stats: as pt_render (the update pass always covers the whole frame);
 * stats->rays counts the update's and the query's rays; a stage that is not run writes nothing (without QUERY `out` may be NULL).
 * Runs like pt_restir_di: on the lane of the next render call, ordered like pt_render_gbuffer; consecutive calls are ordered on the cache
 * whichever lane they use; the lanes are not advanced and pt_get_totals does not count the call.  The context owns the cache -- Capacity
 * keys of 8 bytes and two voxels of 16 bytes each -- allocated on first use and again when Capacity changes.  The cache restarts empty on
 * the first call, with ResetHistory, after pt_set_scene and when Capacity changes.
 * PT_ERR_INVALID_ARG: a null argument; a value outside the ranges of PtSharcSettings; a rect outside RenderSize.  PT_ERR_UNSUPPORTED:
 * IsAntiFireflyEnabled (the filter runs through pt_render_sharc_ex); IsDIEnabled or Denoiser set in the constants.  PT_ERR_STATE: as
 * pt_render. */
PtStatus pt_render_sharc(PtContext *ctx, const PtRect *rect, void *out, int out_is_device, const PtSharcSettings *settings, PtStats *stats);

/* Row N18 -- pt_render_sharc with the frame's direct illumination and the denoiser outputs (the SHARC permutations of
 * Shaders/Raytracing.hlsl with IsDIEnabled and Denoiser != None: :150-163, 302, 311, 318, 376-414; DESIGN.md spec S24), the middle of the
 * reference's default frame GBufferGeneration -> RTXDI -> Raytracing::Render(SHARC) -> DLSS-RR.  di == NULL and outputs == NULL: the call
 * IS pt_render_sharc -- the same cache, restart rules, stages, stats, profiling slots and bits; calls of the two entry points may
 * alternate on one context.  PtGraphicsSettings.IsDIEnabled is ignored (as for pt_render_with_di); the constants' Denoiser stays 0, the
 * mode arrives in `outputs`.
 *   di       DI = Diffuse.rgb + Specular.rgb, e.g. what pt_restir_di* wrote.  A pixel's DI counts where the primary ray hit and
 *            any(DI > 0) (the reference's rule; pt_render_with_di counts every primary surface).  UPDATE: the path's first vertex takes
 *            the DI of the texel its jittered UV falls in, and the second vertex's emission is dropped where that DI counts (unless the
 *            path left through the transmission lobe): the buffers are RenderSize, so with di and UPDATE rect must be NULL or the whole
 *            frame.  QUERY, outputs NULL or Denoiser 1: every sample adds DI at bounce 0 and drops its bounce-1 emission likewise; nothing
 *            is added after the sample average, so a non-finite DI zeroes the pixel.  QUERY, Denoiser 2 / 3: DI is not read, Diffuse /
 *            Specular carry no direct halves, the kept bounce-1 emission is the direct light (the reference's rule).  A QUERY-only call
 *            takes rect-sized buffers, as pt_render_with_di.
 *   outputs  as pt_render_denoiser (spec S13) with res = the query's radiance: Denoiser 1 writes SpecularHitDistance where the primary
 *            ray hit, sample 0 left through a non-diffuse lobe and its bounce-1 ray hit; Denoiser 2 / 3 write out = (primary emission, 1),
 *            Diffuse / Specular on hits.  isDiffuse and the hit distance do not depend on the cache.  A pixel of the hash-grid
 *            visualisation writes only `out`.  outputs->Diffuse / Specular may be di->Diffuse / Specular: the update reads them before
 *            the query writes.
 *   settings->IsAntiFireflyEnabled (row N19, DESIGN.md spec S25; the reference's application sets it, App.cpp:1278): accepted here, with or
 *            without di and outputs, with every Stages mask.  UPDATE: a path's radiance stops going back to earlier vertices where the
 *            luminance of the running segment weight exceeds 2.  RESOLVE: a voxel with a history of 8 samples over 2 frames has this
 *            frame's sums scaled down where their mean luminance exceeds (5 + 5 / samples) max(history luminance, 1).  QUERY does not
 *            read the flag.  The flag has no state: calls with and without it may alternate on one cache.  The arithmetic is this
 *            project's (the SHARC library is not in the reference tree): no parity with the SDK is claimed.
 * Ordering: as pt_render_sharc; with di the lane also waits for everything queued on the context's stream (DI made by pt_restir_di* just
 * before is ordered by the lane's own stream); the DI and output buffers are held to the buffer rotation rule with the lane's frame buffers.
 * PT_ERR_INVALID_ARG also: a null or misaligned DI or output buffer, an output that overlaps another or `out`, a DI buffer that overlaps
 * `out` or an output (other than being Denoiser 2 / 3's Diffuse or Specular itself, as above), Denoiser outside 1..3, di with UPDATE and
 * a partial rect.  On any error nothing is written. */
PtStatus pt_render_sharc_ex(PtContext *ctx, const PtRect *rect, void *out, int out_is_device, const PtSharcSettings *settings,
                            const PtDirectLighting *di, const PtDenoiserOutputs *outputs, PtStats *stats);

/* Row N26 -- the pure path-traced frame through the thin-lens camera (Camera::GenerateThinLensRay, Shaders/Camera.hlsli:43-54, which the
 * reference declares and never calls; DESIGN.md spec S29): pt_render's DEFAULT loop with every sample's primary ray leaving its own point
 * of a lens of radius PtCamera.ApertureRadius towards the pixel's point at view depth |ForwardDirection| (the plane in focus: what
 * CameraController::SetFocusDistance sets).  The lens point is ImportanceSampling::Uniform::GetRay(u).xy of two numbers from a stream of
 * the pixel's own; the bounce loop's random numbers are pt_render's.  ApertureRadius == 0: the frame is pt_render's, bit for bit.  The only
 * entry point that reads ApertureRadius.
 * Camera and aperture come from pt_set_camera, the frame settings (RenderSize, FrameIndex, Bounces, SamplesPerPixel, Russian roulette,
 * ThroughputThreshold) from pt_set_constants.  rect / out / out_is_device / stats: as pt_render_sharc; stats->rays counts every ray
 * traced, each sample's primary ray included.  Runs and is ordered like pt_render_sharc: on the lane of the next render call; the lanes
 * are not advanced and pt_get_totals does not count the call.
 * PT_ERR_INVALID_ARG: a null context or `out`; a rect outside RenderSize; an ApertureRadius that is negative, NaN or infinite.
 * PT_ERR_UNSUPPORTED: IsDIEnabled or Denoiser set in the constants.  PT_ERR_STATE: as pt_render. */
PtStatus pt_render_lens(PtContext *ctx, const PtRect *rect, void *out, int out_is_device, PtStats *stats);

/* Row N27 -- the G-buffer round trip of the reference's frame (DESIGN.md spec S30).
 *
 * pt_render_gbuffer_packed: pt_render_gbuffer with the 13 buffers in the formats the reference's textures have (Source/App.cpp:431-447),
 * 79 bytes per pixel instead of 128:
 *   Position R32G32B32A32_FLOAT 16 B | FlatNormal, GeometricNormal R16G16_SNORM 4 B | LinearDepth, NormalizedDepth R32_FLOAT 4 B |
 *   MotionVector R16G16B16A16_FLOAT 8 B (w = 0) | BaseColorMetalness R8G8B8A8_UNORM 4 B | DiffuseAlbedo, SpecularAlbedo R16G16B16A16_FLOAT
 *   8 B (w = 0) | NormalRoughness R16G16B16A16_SNORM 8 B | IOR R16_FLOAT 2 B | Transmission R8_UNORM 1 B | Radiance R16G16B16A16_FLOAT 8 B
 *   (w = 1).
 * Components in memory order x, y, z, w, little-endian; the conversions are spec S30's (this library's own: D3D's rules are pinned by
 * nothing in the reference tree, no parity with a D3D device is claimed).  In every other respect the contract is pt_render_gbuffer's: the
 * lane and ordering, the miss rule, Transmission only where Metallic < 1, untouched texels left untouched (texel by texel, the 1- and
 * 2-byte ones included), the previous poses, the errors.  Each buffer is aligned to its texel size. */
typedef struct PtGBufferPacked {    /* DEVICE pointers, NULL = not requested; each aligned to its texel: 16 / 8 / 4 / 2 / 1 bytes */
    void *Position, *FlatNormal, *GeometricNormal, *LinearDepth, *NormalizedDepth, *MotionVector,
         *BaseColorMetalness, *DiffuseAlbedo, *SpecularAlbedo, *NormalRoughness, *IOR, *Transmission, *Radiance;
} PtGBufferPacked;
PtStatus pt_render_gbuffer_packed(PtContext *ctx, const PtRect *rect, const PtGBufferPacked *out,
                                  const PtSphere *previous_spheres, const float *previous_rotations);

/* pt_render_from_gbuffer: the pure path-traced frame (the DEFAULT permutation, Denoiser::None) as Shaders/Raytracing.hlsl:103-386 runs
 * it: no primary ray is traced; the first vertex of EVERY sample is the pixel's texel of the eight channels below (:118-148).
 *   Position.w not finite (a miss): out = (Radiance, 1); nothing else is read, no ray is traced.
 *   Otherwise P = Position.xyz with spawn offset Position.w along the decoded FlatNormal; front face = dot(decoded GeometricNormal,
 *   primary direction) < 0; shading normal = NormalRoughness.xyz as stored; material = BaseColor, Metalness, NormalRoughness.w, IOR and
 *   Metalness < 1 ? Transmission : 0 (Transmission is read only there); emission = Radiance.  From the first bounce on the loop, its
 *   random numbers and its result (mean of the samples, 0 where not finite, alpha 1) are pt_render's.
 * Format 0: the float32 layouts of PtGBuffer; with Bounces = 0 and one sample the frame is pt_render's bit for bit, beyond that its
 * first vertex differs from pt_render's by the octahedral round trip of the normals.  Format 1: the layouts of PtGBufferPacked; the
 * picture the reference's arithmetic makes from quantised surfaces (biased against pt_render by design).
 * di (may be NULL): the frame's direct illumination as pt_render_with_di takes it, DI = Diffuse.rgb + Specular.rgb, valid where any
 * component is positive on a hit pixel; where valid the emission at the second vertex is dropped unless the first left through the
 * transmission lobe, and out.rgb += DI after the mean.
 * Buffers are rect.w * rect.h texels, row-major inside the rect.  rect / out / out_is_device / stats: as pt_render_lens; stats->rays
 * counts the rays of the bounce loop (there is no primary ray).  Runs and is ordered like pt_render_lens, on the lane of the next render
 * call; the inputs are held to the rule pt_render_with_di states for its DI buffers: written by pt_render_gbuffer* on the same lane just
 * before (no render call between), they are ordered without a host wait; from anywhere else the frame waits for everything queued on the
 * context's stream before it.  "Written on the same lane" is read from the lane's record of its latest pt_render_gbuffer* call, as
 * pt_restir_di reads it: a pointer that call wrote and that the caller has since overwritten on its own stream is not noticed, so callers
 * keep to the rotation rule (one set of G-buffer buffers per lane, written by this library's pass or made before the window).
 * PT_ERR_INVALID_ARG: a null context, out or input; an unknown Format or a non-zero _pad; a null or misaligned channel or DI buffer; out
 * overlapping an input; a bad rect; IsDIEnabled set without di (with di the constants' flag is not read, as for pt_render_with_di; a
 * Denoiser in the constants is refused by pt_set_constants already).  PT_ERR_STATE: as pt_render. */
typedef struct PtGBufferInput {     /* DEVICE pointers, all required; aligned as PtGBuffer's (Format 0) or PtGBufferPacked's (Format 1) */
    uint32_t Format;                /* 0 float32 layouts, 1 packed layouts */
    uint32_t _pad;                  /* 0 */
    const void *Position, *FlatNormal, *GeometricNormal, *BaseColorMetalness, *NormalRoughness, *IOR, *Transmission, *Radiance;
} PtGBufferInput;
PtStatus pt_render_from_gbuffer(PtContext *ctx, const PtRect *rect, void *out, int out_is_device, const PtGBufferInput *in,
                                const PtDirectLighting *di, PtStats *stats);

/* Test hooks of row N14: the cache as the last pt_render_sharc call left it -- `capacity` keys (uint64, 0 = empty) and resolved voxels
 * (4 x uint32: fixed-point RGB sums, samples | frames << 16 | stale << 24) to HOST memory -- and the reverse, which installs a cache made
 * elsewhere (allocating for `capacity`, a power of two >= 16) as if a call with that Capacity had left it.  Both synchronise.
 * pt_sharc_download: PT_ERR_STATE when there is no cache, PT_ERR_INVALID_ARG when capacity differs from the cache's. */
PtStatus pt_sharc_download(PtContext *ctx, void *keys, void *voxels, uint32_t capacity);
PtStatus pt_sharc_upload(PtContext *ctx, const void *keys, const void *voxels, uint32_t capacity);

/* Row N11 -- the super-resolution stand-in (XeSS::Execute as App::ProcessXeSSSuperResolution drives it, Source/App.cpp:1682-1708; DESIGN.md
 * spec S17): a temporal upscaler of the TAAU / FSR2 family, for XeSS and DLSS-SR, which the reference does not vendor.  From the jittered
 * radiance of a frame rendered at InputSize (PtCamera.Jitter), its G-buffer LinearDepth and MotionVector, to the frame at OutputSize
 * that pt_bloom and pt_tonemap take: a Lanczos-2 resample of the 3 x 3 input pixels around each output pixel in a tone-mapped space,
 * blended with the history reprojected along the nearest-depth tap's motion vector and clamped to the taps' range.
 * On the context's stream (asynchronous), ordered like pt_nrd_composition and pt_bloom: after what is already queued there, before
 * whatever the caller queues next; it adds nothing to pt_get_totals and the render lanes never touch its state.  The context owns the
 * history -- two alternating slots per output pixel of a float4 (tone-space colour, accumulated weight) and a float (depth) --
 * allocated on first use, allocated again when OutputSize changes (which waits for the context's stream only; its size depends on
 * OutputSize alone, so a change of InputSize keeps the allocation) and freed by pt_destroy.  The history restarts on the first call,
 * with Reset, and on any change of InputSize or OutputSize.
 * Not built (spec S17): exposure handling (ExposureScale), a responsive-pixel mask, a bicubic history tap, FSR2's locks and reactive
 * masks, tile and multi-GPU entry points.
 * PT_ERR_INVALID_ARG: a null argument or buffer; a size outside the ranges of PtUpscaleSettings; a Jitter or MaxHistoryWeight that is
 * not finite or out of range; Color or Output not 16-byte aligned, Depth or Velocity not 4-byte aligned; Output overlapping an input. */
typedef struct PtUpscaleTextures {      /* DEVICE pointers; the reference's XeSSResourceType tags */
    const void *Color;                  /* float4, InputSize  (pt_render out / the composed Radiance) */
    const void *Depth;                  /* float,  InputSize  (G-buffer LinearDepth, +inf on a miss) */
    const void *Velocity;               /* float3, InputSize  (G-buffer MotionVector: .xy input pixels, .z view depth) */
    void *Output;                       /* float4, OutputSize */
} PtUpscaleTextures;
PtStatus pt_upscale(PtContext *ctx, const PtUpscaleSettings *settings, const PtUpscaleTextures *textures);
/* xessGetInputResolution plus the reference's Auto rule (Source/App.cpp:1374-1450); needs no context and no GPU.  mode: 0 Auto (by the
 * output's pixel count: <= 1280*800 Native, <= 1920*1200 Quality, <= 2560*1600 Balanced, <= 3840*2400 Performance, else
 * UltraPerformance), 1 Native, 2 Quality, 3 Balanced, 4 Performance, 5 UltraPerformance; scale ratios x 10 = {10, 15, 17, 20, 30};
 * *w = max(1, (out_w * 10 + r10 / 2) / r10) in integer arithmetic, *h likewise.  PT_ERR_INVALID_ARG: an unknown mode, a zero size, a
 * null pointer. */
PtStatus pt_upscale_input_size(uint32_t mode, uint32_t out_w, uint32_t out_h, uint32_t *w, uint32_t *h);

/* Row N12 -- the sharpening stand-in (Streamline's NIS feature as App::ProcessNIS drives it, Source/App.cpp:1710-1721; DESIGN.md spec S18):
 * the reference follows its upscaler with NVIDIA Image Scaling in sharpen mode; the Streamline plugin is not vendored.  A directional
 * unsharp mask in the form of NIS v1's NVSharpen: per texel the luma of a 5 x 5 neighbourhood (coordinates clamped into the image), an
 * edge map over four directions on its inner 3 x 3, a five-tap unsharp mask along the detected directions whose strength and limit
 * fall with the luma, scaled down at hard steps, added to the colour (HdrMode None) or applied as a luma ratio (Linear).  A flat
 * neighbourhood leaves the sanitised colour (NaN -> 0, else clamped to [0, 65504]) unchanged; alpha passes through bit for bit.
 * Color and Output are both at output size (kBufferTypeScalingInputColor / kBufferTypeScalingOutputColor).
 * On the context's stream (asynchronous), ordered like pt_bloom and pt_upscale: after what is already queued there, before whatever
 * the caller queues next.  Stateless: no context state, nothing added to pt_get_totals, the render lanes are never touched.
 * Not built: NIS's scaler mode, HdrMode PQ, tile and multi-GPU entry points.
 * PT_ERR_INVALID_ARG: a null argument or buffer; a size of 0 or above 16384; a Sharpness that is NaN or outside [0, 1]; a buffer not
 * 16-byte aligned; Output overlapping Color, Output == Color included (the pass reads neighbours, so unlike pt_bloom it cannot run in
 * place); an HdrMode above 2.  PT_ERR_UNSUPPORTED: HdrMode 2 (PQ). */
typedef struct PtNisTextures {          /* DEVICE pointers, float4 per texel, Size[0] x Size[1] texels, row-major */
    const void *Color;                  /* kBufferTypeScalingInputColor  (pt_upscale's Output, or the radiance at output size) */
    void *Output;                       /* kBufferTypeScalingOutputColor (what pt_bloom and pt_tonemap take) */
} PtNisTextures;
PtStatus pt_nis_sharpen(PtContext *ctx, const PtNisSettings *settings, const PtNisTextures *textures);

/* Row N29 -- chromatic aberration (the reference's README lists it among the Post-Processing settings, README.md:59, after NVIDIA Image
 * Scaling and before Bloom; the reference tree holds no source for it, so DESIGN.md spec S31 is this project's own and claims no
 * parity): per-channel radial fringing.  Channel c of output texel (x, y) is the bilinear sample, with clamp addressing, of channel c
 * of the sanitised Color (NaN -> 0, else clamped to [0, 65504]) at x + ((x + 0.5) - FocusUV.x W) Offsets[c], and likewise in y: the
 * channel is magnified by 1 + Offsets[c] about the focus.  An offset of 0, or a texel whose centre is the focus, returns the sanitised
 * texel bit for bit; alpha passes through bit for bit.  It sits between pt_nis_sharpen and pt_bloom in the post chain.
 * On the context's stream (asynchronous), ordered like pt_nis_sharpen: after what is already queued there, before whatever the caller
 * queues next.  Stateless: no context state, nothing added to pt_get_totals, the render lanes are never touched.
 * Not built: tile and multi-GPU entry points, a multi-tap spectral variant, barrel distortion, an in-place call, the packed image.
 * PT_ERR_INVALID_ARG: a null argument or buffer; a size of 0 or above 16384; a FocusUV component that is not finite or outside [0, 1];
 * an Offsets component that is not finite or above 1/16 in magnitude; a nonzero _pad; a buffer not 16-byte aligned; Output overlapping
 * Color, Output == Color included (the pass gathers, so it cannot run in place). */
typedef struct PtChromaticAberrationTextures {   /* DEVICE pointers, float4 per texel, Size[0] x Size[1] texels, row-major */
    const void *Color;                  /* pt_nis_sharpen's Output, or the radiance at output size */
    void *Output;                       /* what pt_bloom and pt_tonemap take */
} PtChromaticAberrationTextures;
PtStatus pt_chromatic_aberration(PtContext *ctx, const PtChromaticAberrationSettings *settings, const PtChromaticAberrationTextures *textures);

/* Row N13 -- the frame-interpolation stand-in (DLSS frame generation as App::ProcessDLSSFrameGeneration feeds it, Source/App.cpp:1673-1680;
 * DESIGN.md spec S19): after the tone map the reference tags the G-buffer depth, the motion vectors and the tone-mapped HUD-less colour,
 * and Streamline's DLSS-G plugin, a closed SDK that is not vendored, presents one generated frame between every two rendered ones.
 * Here: the frame at time n - 1/2 from frame n's Color, Depth and MotionVector and frame n - 1's Color and Depth, which the context
 * keeps.  Every render pixel is scattered half its vector back into a motion field through a depth-tested 64-bit min (the nearest
 * surface wins, equal depths go to the lowest pixel index); every output pixel then samples Color half a vector ahead and the previous
 * Color half a vector behind (bilinear), drops a side that is outside the image or, for the previous frame, fails S17's depth test, and
 * averages what is left; a pixel no vector reached copies the previous frame.  Alpha is Color's.  A resting view with equal frames
 * returns them bit for bit.
 * On the context's stream (asynchronous), ordered like pt_bloom, pt_upscale and pt_nis_sharpen.  Nothing is added to pt_get_totals, the
 * render lanes never touch its state.  The context owns two alternating history slots (Color, uint32 x OutputSize, and Depth, float x
 * RenderSize) and the motion field (uint64 x RenderSize): allocated on first use, again when a size changes (which waits for the
 * context's stream only), freed by pt_destroy.
 * *generated (may be NULL) is decided on the host before anything is queued: 0 on a restart -- the first call, Reset, or a change of
 * RenderSize, OutputSize or Format -- where Output is Color bit for bit and the history takes Color and Depth; 1 otherwise.
 * Not built (spec S19): optical flow, a forward scatter from the previous frame's own vectors, inpainting of holes beyond the
 * previous-frame copy, UI / HUD handling, pacing / Reflex, more than one generated frame per pair, tile and multi-GPU entry points.
 * PT_ERR_INVALID_ARG: a null argument or buffer; a size outside the ranges of PtFrameGenSettings; Format > 1; nonzero padding; a
 * buffer not 4-byte aligned; Output overlapping any input, Output == Color included. */
typedef struct PtFrameGenTextures {     /* DEVICE pointers */
    const void *Color;                  /* uint32 per pixel, OutputSize: pt_tonemap's out for frame n (kBufferTypeHUDLessColor) */
    const void *Depth;                  /* float, RenderSize: G-buffer LinearDepth, +inf on a miss (as pt_upscale; the reference tags NormalizedDepth) */
    const void *MotionVector;           /* float3, RenderSize: .xy render pixels towards the previous frame, .z view depth (kBufferTypeMotionVectors) */
    void *Output;                       /* uint32 per pixel, OutputSize: the frame at time n - 1/2 */
} PtFrameGenTextures;
PtStatus pt_frame_gen(PtContext *ctx, const PtFrameGenSettings *settings, const PtFrameGenTextures *textures, uint32_t *generated);

/* Row N15 -- the ray-reconstruction stand-in (DLSS-RR as App::ProcessDLSSRayReconstruction drives it, Source/App.cpp:1654-1671; DESIGN.md
 * spec S21): the reference's default denoiser is one Streamline feature, a closed SDK that is not vendored, which denoises and upscales
 * at once.  Here: from the noisy radiance of pt_render_denoiser's mode 1 at RenderSize, with the G-buffer's LinearDepth, MotionVector,
 * NormalRoughness, DiffuseAlbedo and SpecularAlbedo and mode 1's SpecularHitDistance, to the colour at OutputSize that pt_nis_sharpen,
 * pt_bloom and pt_tonemap take.  Two launches.  Prepare, per render pixel: the sanitised colour divided by DiffuseAlbedo +
 * SpecularAlbedo (a miss is left alone), into S17's tone space; the virtual motion of the specular reflection (the world position
 * rebuilt from LinearDepth as Camera::ReconstructWorldPosition does, pushed along the view ray by the hit distance, through
 * PreviousWorldToProjection) and its weight.  Resolve, per output pixel whose nearest input pixel is a surface: the history read at the
 * surface motion and, where there is one, at the virtual motion (bilinear corners rejected by previous depth and previous normal); the
 * weighted first and second moments of the 5 x 5 input pixels around it, each weight a jitter-aware spatial kernel (wide while the
 * history is short, S17's Lanczos-2 on the inner 3 x 3 once it is long) times edge-stopping terms in depth, normal and roughness; the
 * history clipped to mean +- 1.5 sigma and blended as S17 blends; Output = the inverse tone map times the albedo of the nearest input
 * pixel, alpha from Color.  A pixel whose nearest input pixel is a miss is pt_upscale's pixel, arithmetic unchanged.
 * On the context's stream (asynchronous), ordered like pt_upscale: after what is already queued there, before whatever the caller
 * queues next; it adds nothing to pt_get_totals and the render lanes never touch its state.  The context owns the history -- two
 * alternating slots per output pixel of two float4 (tone-space demodulated colour + accumulated weight, normal + roughness) and a float
 * (depth) -- and three float4 records per render pixel: allocated on first use, again when a size changes (which waits for the
 * context's stream only), freed by pt_destroy.  The history restarts on the first call, with Reset, and on any change of a size.
 * The camera travels by value in PtRayReconstructionSettings (Position and three of PtCamera.Matrices), so the call does not depend
 * on what pt_set_camera last took.
 * Not built (spec S21): a learned model, exposure, transparency and particle layers, DLSS-RR's presets, tile and multi-GPU entry points.
 * PT_ERR_INVALID_ARG: a null argument or buffer; a size outside the ranges of PtRayReconstructionSettings; a Jitter or
 * MaxHistoryWeight that is not finite or out of range; a Position or matrix entry that is not finite; Color, NormalRoughness or Output
 * not 16-byte aligned, another buffer not 4-byte aligned; Output overlapping any input. */
typedef struct PtRayReconstructionTextures { /* DEVICE pointers; the reference's sl::BufferType tags */
    const void *Color;                  /* float4, RenderSize (pt_render_denoiser mode 1's out: kBufferTypeScalingInputColor) */
    const void *Depth;                  /* float,  RenderSize (G-buffer LinearDepth, +inf on a miss, as pt_upscale takes it) */
    const void *MotionVector;           /* float3, RenderSize (.xy render pixels towards the previous frame, .z view depth) */
    const void *NormalRoughness;        /* float4, RenderSize (kBufferTypeNormalRoughness) */
    const void *DiffuseAlbedo;          /* float3, RenderSize (kBufferTypeAlbedo) */
    const void *SpecularAlbedo;         /* float3, RenderSize (kBufferTypeSpecularAlbedo) */
    const void *SpecularHitDistance;    /* float,  RenderSize (kBufferTypeSpecularHitDistance: cleared to 0 by the caller; 0 or not finite = none) */
    void *Output;                       /* float4, OutputSize (kBufferTypeScalingOutputColor) */
} PtRayReconstructionTextures;
PtStatus pt_ray_reconstruction(PtContext *ctx, const PtRayReconstructionSettings *settings, const PtRayReconstructionTextures *textures);
/* Test / tooling hook: the history slot the last pt_ray_reconstruction call wrote, to HOST arrays of OutputSize texels (any may be
 * NULL): history float4 (tone-space demodulated colour, accumulated weight), normal float4 (normal, roughness), depth float.  Waits
 * for the context's stream.  PT_ERR_STATE: no call has been made yet. */
PtStatus pt_ray_reconstruction_history(PtContext *ctx, void *history, void *normal, void *depth);

/* Test / tooling hooks. */
/* Closest hit of n rays against the scene and accel that the NEXT render call renders: o,d = n*3 floats (d unit length), tmin per call.
 * Spheres moved by pt_update_spheres are seen: the lane of the next frame is brought up to date first, as the render call would do it
 * (pending spheres uploaded, boxes refitted -- the render call then does neither again), and its private spheres and refitted tree are
 * what is traced, on the lane's stream, after everything queued on the caller's.  Without an update since pt_set_scene: the master scene.
 * The lane rotation, the frame count and pt_get_totals are not touched.
 * Outputs host arrays t[n], id[n] (id = 0xFFFFFFFF on miss).  use_bvh = 0 runs the device brute-force kernel. */
PtStatus pt_trace_rays(PtContext *ctx, const float *origins, const float *directions, uint32_t n, float tmin,
                       int use_bvh, float *out_t, uint32_t *out_id);
/* As pt_trace_rays through the LBVH, additionally returning per ray {internal nodes visited, spheres tested}
 * (out_visits: n * 2 uint32). */
PtStatus pt_trace_rays_stats(PtContext *ctx, const float *origins, const float *directions, uint32_t n, float tmin,
                             float *out_t, uint32_t *out_id, uint32_t *out_visits);
/* Copy the device BVH to host: nodes[node_count]; leaf child c < 0 refers to Morton-sorted index ~c, whose
 * original sphere id is sorted_id[~c] (pt_accel_download_order: sorted_id[leaf_count]).  As pt_trace_rays, the tree is the one the
 * next render call walks: after pt_update_spheres the refitted private tree of that frame's lane (same links, new boxes).  The leaf
 * order belongs to the topology, which a refit keeps. */
PtStatus pt_accel_download(PtContext *ctx, PtBvhNode *nodes, uint32_t capacity);
PtStatus pt_accel_download_order(PtContext *ctx, uint32_t *sorted_id, uint32_t capacity);
/* Copy the 4-wide, quantised view of the tree that scenes traversed in global memory are walked through:
 * words[node_count * 16], record i at words[16 * i] (the layout is the comment above collapse4_kernel, csrc/pt_lbvh_gpu.hip).  Only
 * the slots of binary nodes at even depth hold a record; the others are zero.  *has_wide = 0, and nothing is copied, when the
 * context has no wide view: an LDS-resident scene, node_count <= 1, or PT_WIDE=0.  Synchronises the context's stream.  Always the view
 * of the tree pt_build_accel made: a lane's refitted private tree has none (it is walked through its binary records).
 * PT_ERR_STATE: no accel; PT_ERR_INVALID_ARG: has_wide null, or a wide view and words null or capacity_nodes < node_count. */
PtStatus pt_accel_download_wide(PtContext *ctx, uint32_t *words, uint32_t capacity_nodes, uint32_t *has_wide);
/* Host LBVH builder (the PT_FLAG_HOST_LBVH path), callable without a context or a GPU, for structural tests:
 * nodes[n-1], sorted_id[n]; returns the tree depth through *depth. */
PtStatus pt_lbvh_build_host(const PtSphere *spheres, uint32_t n, PtBvhNode *nodes, uint32_t *sorted_id, uint32_t *depth);
/* Host SAH builder (the topology pt_build_accel gives small scenes), same outputs. */
PtStatus pt_sah_build_host(const PtSphere *spheres, uint32_t n, PtBvhNode *nodes, uint32_t *sorted_id, uint32_t *depth);
/* Turn per-launch hipEvent profiling on/off (an event pair around every kernel launch, on the stream it runs on). */
PtStatus pt_set_profiling(PtContext *ctx, int enabled);
/* Sum of the per-launch event times recorded since profiling was switched on / last reset, over every render call
 * (synchronises): ms_traverse / traverse_launches = compacting passes (and split-schedule primary / traverse launches),
 * ms_shade / shade_launches = split-schedule shade launches, ms_tail / tail_launches = looping passes. */
PtStatus pt_get_profile(PtContext *ctx, PtStats *profile, int reset);
/* Running totals over every render call since the last reset, accumulated on the device without host
 * synchronisation (rays, paths, pixels, bytes_algorithmic; the timing fields are zero).  Synchronises the stream. */
PtStatus pt_get_totals(PtContext *ctx, PtStats *totals, int reset);
/* Queue sizes of the last spp == 1 frame: sizes[k] = rays in queue k (sizes[0] = path slots).  Returns the number of
 * valid entries through *n (0 if none).  Synchronises the stream. */
PtStatus pt_get_queue_sizes(PtContext *ctx, uint32_t *sizes, uint32_t capacity, uint32_t *n);
/* Reflection beams: running counts, since the last reset (this call's or pt_get_totals'), of the wave64s of 1-spp primary
 * passes that traced in-register bounce-1 rays (*bounce1_waves) and of those whose rays were all served by their block's region list
 * (*listed_waves).  Synchronises the lanes. */
PtStatus pt_get_refl_stats(PtContext *ctx, uint64_t *bounce1_waves, uint64_t *listed_waves, int reset);
/* Device buffers for callers that do not link a GPU runtime themselves (a C++ host written against this header only): the
 * packed tile buffers of pt_render_tiles / pt_gather and the assembled frames of pt_unpack_tiles live in such memory.  The
 * reference's counterpart is the app-owned GPUBuffer / Texture objects handed to the passes (Source/App.cpp:366-368).
 * pt_device_free waits for the frames in flight; pt_download copies device -> host on the context's stream and waits. */
PtStatus pt_device_alloc(PtContext *ctx, uint64_t bytes, void **out_device);
PtStatus pt_device_free(PtContext *ctx, void *device);
PtStatus pt_download(PtContext *ctx, const void *device, void *host, uint64_t bytes);

/* Multi-GPU exchange of HDR tiles (SURVEY 8b `pt_gather`, 8e): one process per GPU, each with its own context; the frame is
 * tile-partitioned (pt_set_partition[_ex] / pt_render_tiles) and the packed tile buffers are gathered to the rank that assembles
 * it.  The reference renders on ONE adapter (Source/DeviceResources.cpp:507 picks a single DXGI adapter); this is the path's
 * multi-GPU extension.  Collectives are RCCL over xGMI; librccl.so is loaded at run time by pt_comm_unique_id / pt_comm_init
 * (PT_ERR_UNSUPPORTED when it cannot be), so single-GPU hosts do not depend on it.
 *   pt_comm_unique_id  rank 0 creates the 128-byte id and ships it to the other ranks (file, socket, launcher environment).
 *   pt_comm_init       collective over all `world` ranks (ncclCommInitRank); the context owns the communicator.
 *   pt_gather          on the context's stream, ordered after the render calls queued before it: every rank other than `root`
 *                      sends `bytes` bytes from send_device (recv_device ignored); the root receives world - 1 parts, the part of
 *                      rank r at recv_device + (r < root ? r : r - 1) * bytes (send_device ignored: its own tiles never travel).
 *                      One grouped ncclSend/ncclRecv exchange, so all inbound links of the root are used at once. */
#define PT_COMM_ID_BYTES 128
PtStatus pt_comm_unique_id(void *id_out);
PtStatus pt_comm_init(PtContext *ctx, const void *id, uint32_t rank, uint32_t world);
PtStatus pt_comm_destroy(PtContext *ctx);
PtStatus pt_gather(PtContext *ctx, const void *send_device, void *recv_device, uint64_t bytes, uint32_t root);

/* Row N23 -- pt_physics_*: a rigid-sphere dynamics step (a stand-in for PhysX as MyScene::Tick drives it, Source/MyScene.ixx:351-396:
 * spring, inverse-square and constant pulls, then PhysX->Tick; DESIGN.md spec S27, whose arithmetic is this project's own -- no parity
 * with PhysX is claimed).  The context owns the state on the device: centre + radius, linear and angular velocity, an orientation
 * quaternion (x, y, z, w) and a PtPhysicsBody record per body, and a tree of its own over the spheres.  A step reads and writes nothing
 * of the scene, the lanes or the frames: the pose reaches the frames on the device through pt_physics_publish (row N24, below), or through
 * the host: pt_physics_download, then pt_update_spheres / pt_update_rotations.
 *   pt_physics_create   replaces any earlier state (validation first: an error keeps it).  lin_vel, ang_vel (n * 3 floats) and rotations
 *                       (n * 4) may be NULL (zero, identity); settings NULL = the defaults of S27; n == 0 is valid.  Builds the tree:
 *                       synchronous.  The first PT_PHYSICS_MAX_LARGE bodies flagged PT_PHYSICS_LARGE do not walk the tree (S27.4).
 *   pt_physics_set_attractors  up to PT_PHYSICS_MAX_ATTRACTORS; pt_physics_create leaves none.
 *   pt_physics_step     `substeps` steps of dt / substeps on the context's stream: asynchronous when report is NULL, except that a step
 *                       which rebuilds the tree (Settings.RebuildInterval) waits for the stream, as the device builder reads the tree's
 *                       depth back.  dt finite and > 0, substeps in [1, 1024]; an error leaves the state untouched.
 *   pt_physics_download waits for the stream; any pointer may be NULL.  spheres: the layout pt_update_spheres takes, rotations: the one
 *                       pt_update_rotations takes; never a NaN (a body whose step is not finite is frozen, S27.7).
 *   pt_physics_destroy  frees the state; pt_destroy calls it. */
PtStatus pt_physics_create(PtContext *ctx, const PtSphere *spheres, const PtPhysicsBody *bodies, const float *lin_vel, const float *ang_vel,
                           const float *rotations, uint32_t n, const PtPhysicsSettings *settings);
PtStatus pt_physics_set_attractors(PtContext *ctx, const PtPhysicsAttractor *attractors, uint32_t n_attractors);
PtStatus pt_physics_step(PtContext *ctx, float dt, uint32_t substeps, PtPhysicsReport *report);
PtStatus pt_physics_download(PtContext *ctx, PtSphere *spheres, float *rotations, float *lin_vel, float *ang_vel);
void pt_physics_destroy(PtContext *ctx);

/* Row N24 -- the simulated pose handed to the frames on the device (DESIGN.md spec S28).
 *   pt_physics_publish  makes the simulation's current pose the pose of every frame from the next render call on: the effect of
 *                       pt_physics_download + pt_update_spheres (+ pt_update_rotations where the context has textures), as one copy
 *                       kernel on the context's stream behind the steps queued so far -- no copy to the host and no host wait (but for
 *                       one-off allocations on first use).  The lanes take the pose on their own streams when they next render or run a
 *                       side pass and refit their trees there; pt_refit_accel is not needed.  May be mixed with pt_update_spheres /
 *                       pt_update_rotations: the newest call wins, per quantity; pt_set_scene forgets what was published.  Images are
 *                       those of the download path bit for bit.  PT_ERR_STATE without pt_physics_create or without scene + accel,
 *                       PT_ERR_INVALID_ARG when the body count is not the scene's sphere count, PT_ERR_UNSUPPORTED with
 *                       PT_FLAG_HOST_LBVH; an empty scene with 0 bodies: PT_OK, nothing done.  An error leaves everything untouched.
 *   pt_render_gbuffer_published  pt_render_gbuffer with the previous pose taken from the device: the pose published before the newest one
 *                       (rotations where the context has textures); after the first publish since pt_physics_create / pt_set_scene the
 *                       current one (no object motion).  PT_ERR_STATE when the scene's newest spheres are not a published pose. */
PtStatus pt_physics_publish(PtContext *ctx);
PtStatus pt_render_gbuffer_published(PtContext *ctx, const PtRect *rect, const PtGBuffer *out);

PtStatus pt_synchronize(PtContext *ctx);

const char *pt_last_error(PtContext *ctx);
const char *pt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PT_API_H */
