/* pt_types.h -- plain-C data layouts of the path-tracing hot path's API surface.
 *
 * These are byte-for-byte the structs the reference host uploads to the GPU for
 * the bounce loop (citations are into /root/reference):
 *
 *   PtMaterial         == Material            Source/Material.ixx:12-20  (== Shaders/Material.hlsli:8-17), 64 B
 *   PtCamera           == Camera              Source/Camera.ixx:16-36    (== Shaders/Camera.hlsli:5-25), 608 B payload
 *   PtSceneData        == SceneData           Source/CommonShaderData.ixx:15-20 (== Shaders/Common.hlsli:7-13), 80 B payload
 *   PtGraphicsSettings == _GraphicsSettings   Source/Raytracing.ixx:151-166 (== Shaders/Raytracing.hlsl:21-39), 80 B
 *   PtNrdCompositionConstants == NRDComposition::Constants   Source/NRDComposition.ixx:23-28 (== Shaders/NRDComposition.hlsl:3-9), 32 B
 *   PtUpscaleSettings     (row N11) the XeSSSettings App::ProcessXeSSSuperResolution fills, plus the output size and the history cap, 32 B
 *   PtNisSettings         (row N12) the sl::NISOptions App::ProcessNIS fills (sharpness, hdrMode; mode is always eSharpen), plus the size, 16 B
 *   PtChromaticAberrationSettings (row N29) the size, FocusUV and Offsets of the README's Chromatic Aberration entry (no source in the reference tree), 32 B
 *   PtRayReconstructionSettings (row N15) the sizes, jitter and reset of sl::DLSSDOptions / sl::Constants plus the camera fields the stand-in reads, 240 B
 *   PtFrameGenSettings    (row N13) the sizes, the packing and the reset flag of the frame-interpolation stand-in (the reference hands DLSS-G only tags), 32 B
 *   PtNrdDenoiseSettings  (row N9) the parts of nrd::CommonSettings / ReblurSettings / RelaxSettings the NRD stand-in reads, 32 B
 *   PtNrdReblurSettings   (row N30) the parts of nrd::CommonSettings / ReblurSettings the ReBLUR stand-in reads, 48 B
 *   PtSharcSettings       (row N14) SHARCSettings (Source/MyAppData.h:256-265) plus the cache's accumulation constants, 48 B
 *   PtLightSamplingSettings (row N16) the local-light sampling mode and the ReGIR settings (Source/MyAppData.h:194-218), 32 B
 *   PtRestirDiCandidates  (row N17) InitialSampling.BRDFSamples and TemporalResampling.BoilingFilter (Source/MyAppData.h:220-235), 16 B
 *   PtRestirDiShading     (row N22) ReSTIRDI_ShadingParameters' final-visibility reuse (the SDK's defaults apply in the reference), 16 B
 *   PtRestirDiSettings    (row N10) the parts of ReSTIRDI_Parameters (Source/MyAppData.h:190-250) the RTXDI stand-in reads, 48 B
 *
 * PtSphere replaces the reference's per-instance ObjectToWorld of the unit
 * geosphere mesh (Source/Scene.ixx:188-203: scale = 2*radius, z flipped): the
 * build intersects analytic spheres, so an instance is (centre, radius).
 *
 * No torch / HIP types appear here; this header is shared by the C-ABI
 * (include/pt_api.h), the C++ host mirror and the CPU oracle (oracle/).
 */
#ifndef PT_TYPES_H
#define PT_TYPES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtSphere {
    float cx, cy, cz; /* world-space centre (render space: PhysX z negated, Scene.ixx:197-199) */
    float r;          /* radius > 0 */
} PtSphere;

/* Source/Material.ixx:10 */
enum { PT_ALPHA_OPAQUE = 0, PT_ALPHA_MASK = 1, PT_ALPHA_BLEND = 2 };

/* Source/Material.ixx:12-20; defaults are BaseColor (0,0,0,1), EmissiveStrength 1,
 * EmissiveColor 0, Metallic 0, Roughness 0.5, IOR 1.5, Transmission 0, Opaque, AlphaCutoff 0.5 */
typedef struct PtMaterial {
    float BaseColor[4];      /*  0 */
    float EmissiveStrength;  /* 16 */
    float EmissiveColor[3];  /* 20 */
    float Metallic;          /* 32 */
    float Roughness;         /* 36 */
    float IOR;               /* 40 */
    float Transmission;      /* 44 */
    uint32_t AlphaMode;      /* 48: not Opaque = non-opaque geometry (Source/Scene.ixx:242-243): every crossing of a ray with the sphere */
    float AlphaCutoff;       /* 52: is a candidate that counts only if BaseColor.a (times the base-colour map's alpha) >= AlphaCutoff --
                                    Mask and Blend alike (Shaders/RaytracingHelpers.hlsli:19-43, ShadingHelpers.hlsli:105-115) */
    uint32_t _pad[2];        /* 56 */
} PtMaterial;

/* Source/Camera.ixx:16-36. The bounce loop reads only Position, Right/Up/Forward
 * (un-normalised, lens scaled), NearDepth, FarDepth and Jitter
 * (Shaders/Raytracing.hlsl:114,126,138; Shaders/Camera.hlsli:27-41).  The G-buffer pass (pt_render_gbuffer)
 * also reads IsNormalizedDepthReversed and three of the matrices (DirectXMath row-vector layout, 16 floats each). */
typedef struct PtCamera {
    uint32_t IsNormalizedDepthReversed; /*   0 */
    float PreviousPosition[3];          /*   4 */
    float Position[3];                  /*  16 */
    float _pad0;                        /*  28 */
    float RightDirection[3];            /*  32 */
    float _pad1;                        /*  44 */
    float UpDirection[3];               /*  48 */
    float _pad2;                        /*  60 */
    float ForwardDirection[3];          /*  64 */
    float ApertureRadius;               /*  76: read by pt_render_lens only (the thin-lens camera, Camera.hlsli:43-54);
                                                pt_set_camera accepts anything, every other entry point ignores it */
    float NearDepth;                    /*  80 */
    float FarDepth;                     /*  84 */
    float Jitter[2];                    /*  88 */
    float Matrices[8][16];              /*  96: PreviousWorldToView, PreviousViewToProjection,
                                                PreviousWorldToProjection, PreviousProjectionToView,
                                                PreviousViewToWorld, WorldToProjection, ProjectionToView,
                                                ViewToWorld -- unused by the bounce loop; pt_render_gbuffer reads
                                                WorldToProjection, PreviousWorldToProjection, PreviousWorldToView */
} PtCamera;

/* Source/CommonShaderData.ixx:15-20. EnvironmentLightColor.a < 0 selects the
 * procedural sky (Shaders/ShadingHelpers.hlsli:25-29).  EnvironmentLightTextureDescriptor
 * != ~0u selects an environment map (ShadingHelpers.hlsli:13-24): it indexes the
 * PtTexture table given to pt_set_textures (this path's descriptor heap), the lookup
 * direction is rotated by the upper 3x3 of EnvironmentLightTransform.  With
 * IsEnvironmentLightTextureCubeMap the descriptor names the first of six consecutive
 * square faces of one size in D3D order (+X, -X, +Y, -Y, +Z, -Z); else a lat-long map. */
typedef struct PtSceneData {
    uint32_t IsStatic;                          /*  0 */
    uint32_t IsEnvironmentLightTextureCubeMap;  /*  4 */
    uint32_t EnvironmentLightTextureDescriptor; /*  8 */
    uint32_t _pad;                              /* 12 */
    float EnvironmentLightColor[4];             /* 16 */
    float EnvironmentLightTransform[12];        /* 32: row-major float3x4 */
} PtSceneData;

/* GPU-side layout of GraphicsSettings, Source/Raytracing.ixx:151-166: HLSL bools are 4 bytes. */
typedef struct PtGraphicsSettings {
    uint32_t RenderSize[2];                      /*  0 */
    uint32_t FrameIndex;                         /*  8 */
    uint32_t Bounces;                            /* 12 */
    uint32_t SamplesPerPixel;                    /* 16 */
    float ThroughputThreshold;                   /* 20: reference default 1e-3 (Raytracing.ixx:33) */
    uint32_t IsRussianRouletteEnabled;           /* 24 */
    uint32_t IsShaderExecutionReorderingEnabled; /* 28: ignored (NV SER has no meaning here) */
    uint32_t IsDIEnabled;                        /* 32: 1 = sphere-light direct illumination of the primary surface (row N4, a stand-in for ReSTIR-DI) */
    uint32_t Denoiser;                           /* 36: must be 0 == Denoiser::None */
    uint32_t _pad0[2];                           /* 40 */
    uint32_t SHARC_Capacity;                     /* 48: SHARC block ignored by pt_set_constants: pt_render_sharc takes PtSharcSettings */
    float SHARC_SceneScale;                      /* 52 */
    float SHARC_RoughnessThreshold;              /* 56 */
    uint32_t SHARC_IsAntiFireflyEnabled;         /* 60 */
    uint32_t SHARC_IsHashGridVisualizationEnabled; /* 64 */
    uint32_t _pad1[3];                           /* 68 */
} PtGraphicsSettings;

/* Row N1 -- textured spheres.  TextureMapInfo mirrors Shaders/Material.hlsli:39-43 / Source/Material.ixx:35-38 (16 bytes);
 * Descriptor indexes the PtTexture array given to pt_set_textures instead of a D3D12 descriptor heap. */
typedef struct PtTextureMapInfo {
    uint32_t Descriptor;              /* ~0u = no texture */
    uint32_t TextureCoordinateIndex;  /* spheres have one UV set: must be 0 */
    uint32_t _pad[2];
} PtTextureMapInfo;

enum { PT_TEXTURE_MAP_BASE_COLOR = 0, PT_TEXTURE_MAP_EMISSIVE_COLOR = 1, PT_TEXTURE_MAP_METALLIC = 2, PT_TEXTURE_MAP_ROUGHNESS = 3,
       PT_TEXTURE_MAP_METALLIC_ROUGHNESS = 4, PT_TEXTURE_MAP_TRANSMISSION = 5, PT_TEXTURE_MAP_NORMAL = 6, PT_TEXTURE_MAP_COUNT = 7 };

/* TextureMapInfoArray of one object (Shaders/Common.hlsli:27, ObjectData::TextureMapInfoArray) */
typedef struct PtObjectTextures {
    PtTextureMapInfo Maps[PT_TEXTURE_MAP_COUNT];
} PtObjectTextures;

/* A decoded image as the reference's TextureHelpers hands it to D3D12 (Source/TextureHelpers.ixx:34-60): 8-bit RGBA texels,
 * either linear (DXGI_FORMAT_R8G8B8A8_UNORM) or sRGB-encoded colour (.._UNORM_SRGB, `forceSRGB`); alpha is always linear. */
typedef struct PtTexture {
    const void *Pixels;    /* host pointer, Width * Height texels of 4 bytes (RGBA8) or 16 bytes (RGBA32_FLOAT), row-major, tightly packed */
    uint32_t Width, Height;
    uint32_t Format;       /* PT_TEXTURE_RGBA8_UNORM | PT_TEXTURE_RGBA8_UNORM_SRGB | PT_TEXTURE_RGBA32_FLOAT */
    uint32_t _pad;
} PtTexture;

/* RGBA32_FLOAT: linear HDR texels, what the reference's EXR/HDR environment maps decode to (DXGI_FORMAT_R32G32B32A32_FLOAT) */
enum { PT_TEXTURE_RGBA8_UNORM = 0, PT_TEXTURE_RGBA8_UNORM_SRGB = 1, PT_TEXTURE_RGBA32_FLOAT = 2 };

/* Display transform parameters (row N3): what App::Impl::ToneMap hands to DirectXTK's ToneMapPostProcess
 * (Source/App.cpp:1731-1757; operator / transfer-function pairs created at Source/App.cpp:760-769). */
typedef struct PtToneMapParams {
    uint32_t Operator;         /* ToneMapPostProcess::Operator: 0 None, 1 Saturate, 2 Reinhard, 3 ACESFilmic */
    uint32_t TransferFunction; /* ToneMapPostProcess::TransferFunction: 0 Linear, 1 SRGB, 2 ST2084 */
    float LinearExposure;      /* SetExposure(stops) -> 2^stops (SDR paths) */
    float PaperWhiteNits;      /* SetST2084Parameter (HDR10 path), default 200 (Source/MyAppData.h:316) */
    uint32_t ColorRotation;    /* SetColorRotation: 0 HDTV_to_UHDTV, 1 DCI_P3_D65_to_UHDTV, 2 HDTV_to_DCI_P3_D65 */
    uint32_t _pad[3];
} PtToneMapParams;

/* Row N8 (pt_nrd_composition): NRDComposition::Constants, uploaded as 8 root constants (Shaders/NRDComposition.hlsl:3-9).
 * App::ProcessNRD passes nrd::ReblurSettings().hitDistanceParameters = {3, 0.1, 20, -25} in ReBLURHitDistance (DESIGN.md spec S14). */
typedef struct PtNrdCompositionConstants {
    uint32_t RenderSize[2];       /*  0 */
    uint32_t Pack;                /*  8: nonzero = pack (before NRD), 0 = compose (after NRD) */
    uint32_t Denoiser;            /* 12: 2 NRDReBLUR, 3 NRDReLAX (Source/Denoiser.ixx) */
    float ReBLURHitDistance[4];   /* 16: hit distance normalisation {A, B, C, D}, read by ReBLUR pack only */
} PtNrdCompositionConstants;

/* Row N9 (pt_nrd_denoise, the NRD stand-in of DESIGN.md spec S15): what App::ProcessNRD hands NRD through nrd::CommonSettings
 * (rectSize, frameIndex, accumulationMode) and the denoiser settings (history lengths), plus the a-trous depth of the stand-in. */
typedef struct PtNrdDenoiseSettings {
    uint32_t RenderSize[2];       /*  0 */
    uint32_t Denoiser;            /*  8: 2 NRDReBLUR, 3 NRDReLAX: the encoding of the In / Out buffers */
    uint32_t AccumulationMode;    /* 12: nrd::AccumulationMode: 0 CONTINUE, 1 RESTART, 2 CLEAR_AND_RESTART */
    uint32_t FrameIndex;          /* 16: accepted, not read by S15 */
    uint32_t MaxDiffuseFrames;    /* 20: 0 -> 30 */
    uint32_t MaxSpecularFrames;   /* 24: 0 -> 30 */
    uint32_t AtrousIterations;    /* 28: 0 -> 5, at most 8 */
} PtNrdDenoiseSettings;

/* Row N30 (pt_nrd_reblur, the ReBLUR stand-in of DESIGN.md spec S32): what App::ProcessNRD hands NRD through nrd::CommonSettings
 * (rectSize, frameIndex, accumulationMode) and the history lengths and blur radii of nrd::ReblurSettings.  0 = the default; the defaults
 * are nrd::ReblurSettings' (maxAccumulatedFrameNum 30, maxFastAccumulatedFrameNum 6, historyFixFrameNum 3, minBlurRadius 1, maxBlurRadius
 * 30) as recollected: the reference does not vendor the NRD SDK. */
typedef struct PtNrdReblurSettings {
    uint32_t RenderSize[2];            /*  0: 1..16384 each */
    uint32_t AccumulationMode;         /*  8: nrd::AccumulationMode: 0 CONTINUE, 1 RESTART, 2 CLEAR_AND_RESTART */
    uint32_t FrameIndex;               /* 12: read: it turns the blur's tap pattern */
    uint32_t MaxAccumulatedFrames;     /* 16: 0 -> 30 */
    uint32_t MaxFastAccumulatedFrames; /* 20: 0 -> 6; at most MaxAccumulatedFrames */
    uint32_t HistoryFixFrames;         /* 24: 0 -> 3 */
    float MinBlurRadius;               /* 28: pixels; 0 -> 1; finite, >= 0, at most MaxBlurRadius */
    float MaxBlurRadius;               /* 32: pixels; 0 -> 30; finite, >= 0, at most 64 */
    uint32_t _pad[3];                  /* 36: must be 0 */
} PtNrdReblurSettings;

/* Row N10 (pt_restir_di, the RTXDI stand-in of DESIGN.md spec S16): what RTXDI::SetConstants hands the DI passes (Source/App.cpp:1187-1227;
 * defaults of Source/MyAppData.h:190-250). */
typedef struct PtRestirDiSettings {
    uint32_t RenderSize[2];          /*  0: 1..16384 each */
    uint32_t FrameIndex;             /*  8: seeds the pass's own RNG streams */
    uint32_t ResetHistory;           /* 12: nonzero = ignore the history (m_resetHistory) */
    uint32_t InitialSamples;         /* 16: 0 -> 8, at most 32 (InitialSampling.LocalLight.Samples) */
    uint32_t EnableTemporal;         /* 20: 0 / 1 */
    uint32_t TemporalBiasCorrection; /* 24: 0 Off, 1 Basic, 3 Raytraced; 2 (Pairwise): pt_restir_di_full only, elsewhere PT_ERR_UNSUPPORTED */
    uint32_t MaxHistoryLength;       /* 28: 0 -> 20; a history reservoir's M is capped at this many times the current M */
    uint32_t EnableSpatial;          /* 32: 0 / 1 */
    uint32_t SpatialBiasCorrection;  /* 36: as the temporal field */
    uint32_t SpatialSamples;         /* 40: 0 -> 1, at most 32 */
    float SpatialRadius;             /* 44: pixels; 0 -> 32; finite and >= 0 (radii above 16384 act as 16384) */
} PtRestirDiSettings;

/* Row N16 (pt_restir_di_sampled, DESIGN.md spec S22): the local-light sampling mode of ReSTIRDI_LocalLightSamplingMode and the sizes of
 * the presampled structures (Source/MyAppData.h:194-218; defaults of the RTXDI SDK as recollected).  0 = the default. */
typedef struct PtLightSamplingSettings {
    uint32_t Mode;                /*  0: PT_LIGHT_SAMPLING_UNIFORM / _POWER_RIS / _REGIR_RIS (the reference's default is ReGIR_RIS) */
    uint32_t TileSize;            /*  4: entries of a Power_RIS tile; 0 -> 1024, at most 8192 */
    uint32_t TileCount;           /*  8: Power_RIS tiles; 0 -> 128, at most 1024 */
    uint32_t ReGIRGridSize;       /* 12: cells per axis of the cube around the camera; 0 -> 16, at most 32 */
    uint32_t ReGIRLightsPerCell;  /* 16: 0 -> 512, at most 1024 */
    uint32_t ReGIRBuildSamples;   /* 20: 0 -> 8, at most 32 */
    float ReGIRCellSize;          /* 24: 0 -> 1; otherwise finite, 0.1 .. 10 */
    uint32_t _pad;                /* 28: must be 0 */
} PtLightSamplingSettings;

enum { PT_LIGHT_SAMPLING_UNIFORM = 0, PT_LIGHT_SAMPLING_POWER_RIS = 1, PT_LIGHT_SAMPLING_REGIR_RIS = 2 };

/* Row N17 (pt_restir_di_ex, DESIGN.md spec S23): the BRDF candidates of initial sampling and the boiling filter of temporal resampling
 * (Source/MyAppData.h:220-221, 229-235).  All zero = both off. */
typedef struct PtRestirDiCandidates {
    uint32_t BrdfSamples;           /*  0: 0 .. 8; 0 = none; the reference's default is 1 (InitialSampling.BRDFSamples) */
    uint32_t EnableBoilingFilter;   /*  4: 0 / 1; the reference's default is 1 */
    float    BoilingFilterStrength; /*  8: finite, 0 .. 1; the reference's default is 0.2; read only when the filter is enabled */
    uint32_t _pad;                  /* 12: must be 0 */
} PtRestirDiCandidates;

/* Row N22 (pt_restir_di_full, DESIGN.md spec S26): final shading's reuse of a sample's visibility (DIFinalShading.hlsl:32-56,
 * reuseFinalVisibility; the reference leaves the SDK's shading parameters at their defaults, Source/RTXDI.ixx:134 -- on, 4 and 16 as
 * recollected).  The two limits are literal: 0 does not stand for a default.  All zero = off. */
typedef struct PtRestirDiShading {
    uint32_t ReuseFinalVisibility;       /*  0: 0 / 1 */
    uint32_t FinalVisibilityMaxAge;      /*  4: frames, at most 255; 0 = only a sample drawn by this call */
    float    FinalVisibilityMaxDistance; /*  8: pixels, finite and >= 0; 0 = only the pixel that drew the sample */
    uint32_t _pad;                       /* 12: must be 0 */
} PtRestirDiShading;

/* Row N11 (pt_upscale, the XeSS / DLSS-SR stand-in of DESIGN.md spec S17): XeSSSettings as App::ProcessXeSSSuperResolution fills it
 * (Source/App.cpp:1685-1690; InputSize, Jitter, Reset), the output size XeSS is created with, and the stand-in's history cap. */
typedef struct PtUpscaleSettings {
    uint32_t InputSize[2];        /*  0: RenderSize of the inputs, 1..16384 each */
    uint32_t OutputSize[2];       /*  8: InputSize <= OutputSize <= 4 * InputSize per axis, at most 16384 */
    float Jitter[2];              /* 16: what the host hands XeSS: -PtCamera.Jitter, in pixels of the input; finite, |.| <= 1 */
    uint32_t Reset;               /* 24: nonzero = ignore the history (m_resetHistory) */
    float MaxHistoryWeight;       /* 28: 0 -> 16; finite, 1..256 */
} PtUpscaleSettings;

/* Row N12 (pt_nis_sharpen, the NIS stand-in of DESIGN.md spec S18): sl::NISOptions as App::ProcessNIS fills it (Source/App.cpp:1710-1721;
 * mode = eSharpen always) and the size of the two tagged buffers, which is the output size. */
typedef struct PtNisSettings {
    uint32_t Size[2];             /*  0: texels of Color and Output, 1..16384 each */
    float Sharpness;              /*  8: PostProcessing.NIS.Sharpness, in [0, 1]; the reference's default is 0.5 */
    uint32_t HdrMode;             /* 12: sl::NISHDR: 0 None (what the reference passes), 1 Linear; 2 PQ is PT_ERR_UNSUPPORTED */
} PtNisSettings;

/* Row N29 (pt_chromatic_aberration, DESIGN.md spec S31): the reference's README lists Chromatic Aberration among its post-processing
 * settings, between NVIDIA Image Scaling and Bloom; the reference tree holds no source for it, so the fields are this project's own. */
typedef struct PtChromaticAberrationSettings {
    uint32_t Size[2];             /*  0: texels of Color and Output, 1..16384 each */
    float FocusUV[2];             /*  8: the point the fringes radiate from, each in [0, 1]; (0.5, 0.5) is the image centre */
    float Offsets[3];             /* 16: the signed factor k of r, g, b: a channel is magnified by 1 + k about the focus; |k| <= 1/16 */
    uint32_t _pad;                /* 28: must be 0 */
} PtChromaticAberrationSettings;

/* Row N13 (pt_frame_gen, the DLSS-G stand-in of DESIGN.md spec S19): App::ProcessDLSSFrameGeneration (Source/App.cpp:1673-1680) only
 * tags resources; their sizes, the packing of the tone-mapped colour and m_resetHistory travel here. */
typedef struct PtFrameGenSettings {
    uint32_t RenderSize[2];       /*  0: size of Depth and MotionVector, 1..16384 each */
    uint32_t OutputSize[2];       /*  8: size of Color and Output; RenderSize <= OutputSize <= 4 * RenderSize per axis, at most 16384 */
    uint32_t Format;              /* 16: 0 R8G8B8A8_UNORM, 1 R10G10B10A2_UNORM: pt_tonemap's two packings */
    uint32_t Reset;               /* 20: nonzero = ignore the history (m_resetHistory) */
    uint32_t _pad[2];             /* 24: must be 0 */
} PtFrameGenSettings;

/* Row N15 (pt_ray_reconstruction, the DLSS-RR stand-in of DESIGN.md spec S21): what App::ProcessDLSSRayReconstruction hands Streamline
 * in sl::DLSSDOptions and sl::Constants (Source/App.cpp:1654-1671): the sizes, the jitter, the reset flag, and -- by value, in place of
 * worldToCameraView / cameraViewToWorld and the constants' matrices -- the camera fields the stand-in reads, as PtCamera holds them. */
typedef struct PtRayReconstructionSettings {
    uint32_t RenderSize[2];               /*   0: 1..16384 each */
    uint32_t OutputSize[2];               /*   8: RenderSize <= OutputSize <= 4 * RenderSize per axis, at most 16384 */
    float Jitter[2];                      /*  16: -PtCamera.Jitter, in render pixels, as PtUpscaleSettings.Jitter; finite, |.| <= 1 */
    uint32_t Reset;                       /*  24: nonzero = ignore the history (m_resetHistory) */
    float MaxHistoryWeight;               /*  28: 0 -> 16; finite, 1..256 */
    float Position[3];                    /*  32: PtCamera.Position */
    float _pad;                           /*  44 */
    float ProjectionToView[16];           /*  48: PtCamera.Matrices[6] */
    float ViewToWorld[16];                /* 112: PtCamera.Matrices[7] */
    float PreviousWorldToProjection[16];  /* 176: PtCamera.Matrices[2] */
} PtRayReconstructionSettings;

/* Row N14 (pt_render_sharc, the SHARC stand-in of DESIGN.md spec S20): SHARCSettings as Raytracing::Render(..., SHARC&, SHARCSettings) takes
 * them (Source/MyAppData.h:256-265, Source/Raytracing.ixx:114-148), the cache's accumulation constants and the stages of the call. */
typedef struct PtSharcSettings {
    uint32_t Capacity;                        /*  0: slots of the hash map; 0 -> 1 << 22; a power of two, 16 .. 1 << 28 */
    uint32_t DownscaleFactor;                 /*  4: the update pass traces (W / f) x (H / f) paths; 0 -> 4; 1 .. 4 */
    float SceneScale;                         /*  8: 0 -> 50; 5 .. 100 */
    float RoughnessThreshold;                 /* 12: 0 .. 1: the update pass's surfaces are at least this rough */
    uint32_t AccumulationFrames;              /* 16: 0 -> 10; 1 .. 255 */
    uint32_t MaxStaleFrames;                  /* 20: 0 -> 64; 1 .. 254 */
    uint32_t IsAntiFireflyEnabled;            /* 24: nonzero = the anti-firefly filter of spec S25 in the update and the resolve
                                               *     (pt_render_sharc_ex; pt_render_sharc -> PT_ERR_UNSUPPORTED) */
    uint32_t IsHashGridVisualizationEnabled;  /* 28: a pixel whose path met the cache shows a colour of its primary hit's cell */
    uint32_t ResetHistory;                    /* 32: nonzero = the cache restarts empty with this call */
    uint32_t Stages;                          /* 36: PT_SHARC_UPDATE | PT_SHARC_RESOLVE | PT_SHARC_QUERY; 0 -> all three */
    uint32_t _pad[2];                         /* 40: must be 0 */
} PtSharcSettings;

enum { PT_SHARC_UPDATE = 1, PT_SHARC_RESOLVE = 2, PT_SHARC_QUERY = 4 };

/* Row N23 -- pt_physics_* (a rigid-sphere dynamics stand-in for PhysX, DESIGN.md spec S27). */
typedef struct PtPhysicsBody {
    float InvMass;       /*  0: 1 / mass; 0 = immovable (moves with its velocity only, takes no force and no impulse) */
    uint32_t Flags;      /*  4: PT_PHYSICS_SPRING | PT_PHYSICS_LARGE | PT_PHYSICS_DISABLED */
    float SpringY0;      /*  8: SPRING: the rest height ... */
    float SpringOmega2;  /* 12: ... and 4 pi^2 / T^2 */
} PtPhysicsBody;

enum { PT_PHYSICS_SPRING = 1, PT_PHYSICS_LARGE = 2, PT_PHYSICS_DISABLED = 4 };

typedef struct PtPhysicsSettings {
    uint32_t Iterations;       /*  0: Jacobi velocity iterations; 0 -> 4; at most 64 */
    uint32_t RebuildInterval;  /*  4: the tree is rebuilt every so many steps (which waits for the stream); 0 = never (refit only) */
    float Restitution;         /*  8: e, 0 .. 1 (the reference's material: 0.6) */
    float Friction;            /* 12: mu >= 0 (0.5) */
    float Baumgarte;           /* 16: beta, 0 .. 1 (0.2) */
    float Slop;                /* 20: penetration left uncorrected, >= 0 (0.005) */
    float BounceThreshold;     /* 24: approach speed above which a contact bounces, >= 0 (2: PhysX's default, 0.2 x its speed scale of 10) */
    uint32_t _pad;             /* 28: must be 0 */
} PtPhysicsSettings;

typedef struct PtPhysicsAttractor {
    uint32_t Body;      /*  0: the body that attracts */
    uint32_t Kind;      /*  4: PT_PHYSICS_INVERSE_SQUARE (Strength = GM, acceleration GM / d^2) or PT_PHYSICS_CONSTANT (Strength = acceleration) */
    float Strength;     /*  8: finite */
    uint32_t Target;    /* 12: PT_PHYSICS_ALL_BODIES (all but Body itself) or the one body attracted */
} PtPhysicsAttractor;

enum { PT_PHYSICS_INVERSE_SQUARE = 0, PT_PHYSICS_CONSTANT = 1 };
#define PT_PHYSICS_ALL_BODIES 0xFFFFFFFFu
#define PT_PHYSICS_MAX_ATTRACTORS 4
#define PT_PHYSICS_MAX_LARGE 64

typedef struct PtPhysicsReport {
    uint32_t Contacts;  /*  0: pairs in contact, summed over the call's substeps */
    uint32_t Clamped;   /*  4: nonzero = some contribution to an accumulator was clamped (sticky over the substeps) */
    uint32_t Frozen;    /*  8: bodies frozen by a non-finite result in this call */
    uint32_t Steps;     /* 12: substeps made since pt_physics_create, this call's included */
} PtPhysicsReport;

/* Pixel rectangle in render-target coordinates. */
typedef struct PtRect {
    uint32_t x, y, w, h;
} PtRect;

#ifdef __cplusplus
} /* extern "C" */
#endif

#ifdef __cplusplus
static_assert(sizeof(PtSphere) == 16, "PtSphere layout");
static_assert(sizeof(PtPhysicsBody) == 16 && sizeof(PtPhysicsSettings) == 32 && sizeof(PtPhysicsAttractor) == 16 && sizeof(PtPhysicsReport) == 16, "pt_physics layouts");
static_assert(sizeof(PtMaterial) == 64, "PtMaterial layout");
static_assert(sizeof(PtCamera) == 608, "PtCamera layout");
static_assert(sizeof(PtSceneData) == 80, "PtSceneData layout");
static_assert(sizeof(PtGraphicsSettings) == 80, "PtGraphicsSettings layout");
static_assert(sizeof(PtToneMapParams) == 32, "PtToneMapParams layout");
static_assert(sizeof(PtTextureMapInfo) == 16 && sizeof(PtObjectTextures) == 112, "TextureMapInfoArray layout");
static_assert(sizeof(PtNrdCompositionConstants) == 32 && offsetof(PtNrdCompositionConstants, Pack) == 8
              && offsetof(PtNrdCompositionConstants, Denoiser) == 12 && offsetof(PtNrdCompositionConstants, ReBLURHitDistance) == 16,
              "NRDComposition::Constants layout");
static_assert(sizeof(PtNrdDenoiseSettings) == 32 && offsetof(PtNrdDenoiseSettings, Denoiser) == 8 && offsetof(PtNrdDenoiseSettings, AccumulationMode) == 12
              && offsetof(PtNrdDenoiseSettings, MaxDiffuseFrames) == 20 && offsetof(PtNrdDenoiseSettings, AtrousIterations) == 28, "PtNrdDenoiseSettings layout");
static_assert(sizeof(PtNrdReblurSettings) == 48 && offsetof(PtNrdReblurSettings, AccumulationMode) == 8 && offsetof(PtNrdReblurSettings, FrameIndex) == 12
              && offsetof(PtNrdReblurSettings, MaxAccumulatedFrames) == 16 && offsetof(PtNrdReblurSettings, MaxFastAccumulatedFrames) == 20
              && offsetof(PtNrdReblurSettings, HistoryFixFrames) == 24 && offsetof(PtNrdReblurSettings, MinBlurRadius) == 28
              && offsetof(PtNrdReblurSettings, MaxBlurRadius) == 32 && offsetof(PtNrdReblurSettings, _pad) == 36, "PtNrdReblurSettings layout");
static_assert(sizeof(PtRestirDiSettings) == 48 && offsetof(PtRestirDiSettings, ResetHistory) == 12 && offsetof(PtRestirDiSettings, TemporalBiasCorrection) == 24
              && offsetof(PtRestirDiSettings, EnableSpatial) == 32 && offsetof(PtRestirDiSettings, SpatialRadius) == 44, "PtRestirDiSettings layout");
static_assert(sizeof(PtLightSamplingSettings) == 32 && offsetof(PtLightSamplingSettings, TileSize) == 4 && offsetof(PtLightSamplingSettings, TileCount) == 8
              && offsetof(PtLightSamplingSettings, ReGIRGridSize) == 12 && offsetof(PtLightSamplingSettings, ReGIRLightsPerCell) == 16
              && offsetof(PtLightSamplingSettings, ReGIRBuildSamples) == 20 && offsetof(PtLightSamplingSettings, ReGIRCellSize) == 24
              && offsetof(PtLightSamplingSettings, _pad) == 28, "PtLightSamplingSettings layout");
static_assert(sizeof(PtRestirDiCandidates) == 16 && offsetof(PtRestirDiCandidates, BoilingFilterStrength) == 8, "PtRestirDiCandidates layout");
static_assert(sizeof(PtRestirDiShading) == 16 && offsetof(PtRestirDiShading, FinalVisibilityMaxAge) == 4 && offsetof(PtRestirDiShading, FinalVisibilityMaxDistance) == 8
              && offsetof(PtRestirDiShading, _pad) == 12, "PtRestirDiShading layout");
static_assert(sizeof(PtUpscaleSettings) == 32 && offsetof(PtUpscaleSettings, OutputSize) == 8 && offsetof(PtUpscaleSettings, Jitter) == 16
              && offsetof(PtUpscaleSettings, Reset) == 24 && offsetof(PtUpscaleSettings, MaxHistoryWeight) == 28, "PtUpscaleSettings layout");
static_assert(sizeof(PtNisSettings) == 16 && offsetof(PtNisSettings, Sharpness) == 8 && offsetof(PtNisSettings, HdrMode) == 12, "PtNisSettings layout");
static_assert(sizeof(PtChromaticAberrationSettings) == 32 && offsetof(PtChromaticAberrationSettings, FocusUV) == 8 && offsetof(PtChromaticAberrationSettings, Offsets) == 16
              && offsetof(PtChromaticAberrationSettings, _pad) == 28, "PtChromaticAberrationSettings layout");
static_assert(sizeof(PtFrameGenSettings) == 32 && offsetof(PtFrameGenSettings, OutputSize) == 8 && offsetof(PtFrameGenSettings, Format) == 16
              && offsetof(PtFrameGenSettings, Reset) == 20 && offsetof(PtFrameGenSettings, _pad) == 24, "PtFrameGenSettings layout");
static_assert(sizeof(PtSharcSettings) == 48 && offsetof(PtSharcSettings, SceneScale) == 8 && offsetof(PtSharcSettings, AccumulationFrames) == 16
              && offsetof(PtSharcSettings, ResetHistory) == 32 && offsetof(PtSharcSettings, Stages) == 36, "PtSharcSettings layout");
static_assert(sizeof(PtRayReconstructionSettings) == 240 && offsetof(PtRayReconstructionSettings, Jitter) == 16 && offsetof(PtRayReconstructionSettings, Reset) == 24
              && offsetof(PtRayReconstructionSettings, MaxHistoryWeight) == 28 && offsetof(PtRayReconstructionSettings, Position) == 32
              && offsetof(PtRayReconstructionSettings, ProjectionToView) == 48 && offsetof(PtRayReconstructionSettings, ViewToWorld) == 112
              && offsetof(PtRayReconstructionSettings, PreviousWorldToProjection) == 176, "PtRayReconstructionSettings layout");
#else
_Static_assert(sizeof(PtSphere) == 16, "PtSphere layout");
_Static_assert(sizeof(PtPhysicsBody) == 16 && sizeof(PtPhysicsSettings) == 32 && sizeof(PtPhysicsAttractor) == 16 && sizeof(PtPhysicsReport) == 16, "pt_physics layouts");
_Static_assert(sizeof(PtMaterial) == 64, "PtMaterial layout");
_Static_assert(sizeof(PtCamera) == 608, "PtCamera layout");
_Static_assert(sizeof(PtSceneData) == 80, "PtSceneData layout");
_Static_assert(sizeof(PtGraphicsSettings) == 80, "PtGraphicsSettings layout");
_Static_assert(sizeof(PtNrdCompositionConstants) == 32 && offsetof(PtNrdCompositionConstants, Pack) == 8
               && offsetof(PtNrdCompositionConstants, Denoiser) == 12 && offsetof(PtNrdCompositionConstants, ReBLURHitDistance) == 16,
               "NRDComposition::Constants layout");
_Static_assert(sizeof(PtNrdDenoiseSettings) == 32 && offsetof(PtNrdDenoiseSettings, Denoiser) == 8 && offsetof(PtNrdDenoiseSettings, AccumulationMode) == 12
               && offsetof(PtNrdDenoiseSettings, MaxDiffuseFrames) == 20 && offsetof(PtNrdDenoiseSettings, AtrousIterations) == 28, "PtNrdDenoiseSettings layout");
_Static_assert(sizeof(PtNrdReblurSettings) == 48 && offsetof(PtNrdReblurSettings, AccumulationMode) == 8 && offsetof(PtNrdReblurSettings, FrameIndex) == 12
               && offsetof(PtNrdReblurSettings, MaxAccumulatedFrames) == 16 && offsetof(PtNrdReblurSettings, MaxFastAccumulatedFrames) == 20
               && offsetof(PtNrdReblurSettings, HistoryFixFrames) == 24 && offsetof(PtNrdReblurSettings, MinBlurRadius) == 28
               && offsetof(PtNrdReblurSettings, MaxBlurRadius) == 32 && offsetof(PtNrdReblurSettings, _pad) == 36, "PtNrdReblurSettings layout");
_Static_assert(sizeof(PtRestirDiSettings) == 48 && offsetof(PtRestirDiSettings, ResetHistory) == 12 && offsetof(PtRestirDiSettings, TemporalBiasCorrection) == 24
               && offsetof(PtRestirDiSettings, EnableSpatial) == 32 && offsetof(PtRestirDiSettings, SpatialRadius) == 44, "PtRestirDiSettings layout");
_Static_assert(sizeof(PtLightSamplingSettings) == 32 && offsetof(PtLightSamplingSettings, TileSize) == 4 && offsetof(PtLightSamplingSettings, TileCount) == 8
               && offsetof(PtLightSamplingSettings, ReGIRGridSize) == 12 && offsetof(PtLightSamplingSettings, ReGIRLightsPerCell) == 16
               && offsetof(PtLightSamplingSettings, ReGIRBuildSamples) == 20 && offsetof(PtLightSamplingSettings, ReGIRCellSize) == 24
               && offsetof(PtLightSamplingSettings, _pad) == 28, "PtLightSamplingSettings layout");
_Static_assert(sizeof(PtRestirDiCandidates) == 16 && offsetof(PtRestirDiCandidates, BoilingFilterStrength) == 8, "PtRestirDiCandidates layout");
_Static_assert(sizeof(PtRestirDiShading) == 16 && offsetof(PtRestirDiShading, FinalVisibilityMaxAge) == 4 && offsetof(PtRestirDiShading, FinalVisibilityMaxDistance) == 8
               && offsetof(PtRestirDiShading, _pad) == 12, "PtRestirDiShading layout");
_Static_assert(sizeof(PtUpscaleSettings) == 32 && offsetof(PtUpscaleSettings, OutputSize) == 8 && offsetof(PtUpscaleSettings, Jitter) == 16
               && offsetof(PtUpscaleSettings, Reset) == 24 && offsetof(PtUpscaleSettings, MaxHistoryWeight) == 28, "PtUpscaleSettings layout");
_Static_assert(sizeof(PtNisSettings) == 16 && offsetof(PtNisSettings, Sharpness) == 8 && offsetof(PtNisSettings, HdrMode) == 12, "PtNisSettings layout");
_Static_assert(sizeof(PtChromaticAberrationSettings) == 32 && offsetof(PtChromaticAberrationSettings, FocusUV) == 8 && offsetof(PtChromaticAberrationSettings, Offsets) == 16
               && offsetof(PtChromaticAberrationSettings, _pad) == 28, "PtChromaticAberrationSettings layout");
_Static_assert(sizeof(PtFrameGenSettings) == 32 && offsetof(PtFrameGenSettings, OutputSize) == 8 && offsetof(PtFrameGenSettings, Format) == 16
               && offsetof(PtFrameGenSettings, Reset) == 20 && offsetof(PtFrameGenSettings, _pad) == 24, "PtFrameGenSettings layout");
_Static_assert(sizeof(PtSharcSettings) == 48 && offsetof(PtSharcSettings, SceneScale) == 8 && offsetof(PtSharcSettings, AccumulationFrames) == 16
               && offsetof(PtSharcSettings, ResetHistory) == 32 && offsetof(PtSharcSettings, Stages) == 36, "PtSharcSettings layout");
_Static_assert(sizeof(PtRayReconstructionSettings) == 240 && offsetof(PtRayReconstructionSettings, Jitter) == 16 && offsetof(PtRayReconstructionSettings, Reset) == 24
               && offsetof(PtRayReconstructionSettings, MaxHistoryWeight) == 28 && offsetof(PtRayReconstructionSettings, Position) == 32
               && offsetof(PtRayReconstructionSettings, ProjectionToView) == 48 && offsetof(PtRayReconstructionSettings, ViewToWorld) == 112
               && offsetof(PtRayReconstructionSettings, PreviousWorldToProjection) == 176, "PtRayReconstructionSettings layout");
#endif

#endif /* PT_TYPES_H */
