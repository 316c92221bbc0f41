"""ctypes / numpy mirrors of include/pt_types.h and include/pt_api.h."""
import ctypes as C

import numpy as np


class PtSphere(C.Structure):
    _fields_ = [("cx", C.c_float), ("cy", C.c_float), ("cz", C.c_float), ("r", C.c_float)]


class PtMaterial(C.Structure):
    _fields_ = [
        ("BaseColor", C.c_float * 4), ("EmissiveStrength", C.c_float), ("EmissiveColor", C.c_float * 3),
        ("Metallic", C.c_float), ("Roughness", C.c_float), ("IOR", C.c_float), ("Transmission", C.c_float),
        ("AlphaMode", C.c_uint32), ("AlphaCutoff", C.c_float), ("_pad", C.c_uint32 * 2),
    ]


class PtCamera(C.Structure):
    _fields_ = [
        ("IsNormalizedDepthReversed", C.c_uint32), ("PreviousPosition", C.c_float * 3), ("Position", C.c_float * 3),
        ("_pad0", C.c_float), ("RightDirection", C.c_float * 3), ("_pad1", C.c_float), ("UpDirection", C.c_float * 3),
        ("_pad2", C.c_float), ("ForwardDirection", C.c_float * 3), ("ApertureRadius", C.c_float),
        ("NearDepth", C.c_float), ("FarDepth", C.c_float), ("Jitter", C.c_float * 2), ("Matrices", (C.c_float * 16) * 8),
    ]


class PtSceneData(C.Structure):
    _fields_ = [
        ("IsStatic", C.c_uint32), ("IsEnvironmentLightTextureCubeMap", C.c_uint32),
        ("EnvironmentLightTextureDescriptor", C.c_uint32), ("_pad", C.c_uint32),
        ("EnvironmentLightColor", C.c_float * 4), ("EnvironmentLightTransform", C.c_float * 12),
    ]


class PtGraphicsSettings(C.Structure):
    _fields_ = [
        ("RenderSize", C.c_uint32 * 2), ("FrameIndex", C.c_uint32), ("Bounces", C.c_uint32), ("SamplesPerPixel", C.c_uint32),
        ("ThroughputThreshold", C.c_float), ("IsRussianRouletteEnabled", C.c_uint32),
        ("IsShaderExecutionReorderingEnabled", C.c_uint32), ("IsDIEnabled", C.c_uint32), ("Denoiser", C.c_uint32),
        ("_pad0", C.c_uint32 * 2), ("SHARC_Capacity", C.c_uint32), ("SHARC_SceneScale", C.c_float),
        ("SHARC_RoughnessThreshold", C.c_float), ("SHARC_IsAntiFireflyEnabled", C.c_uint32),
        ("SHARC_IsHashGridVisualizationEnabled", C.c_uint32), ("_pad1", C.c_uint32 * 3),
    ]


class PtRect(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


# Row N6 (pt_render_gbuffer): the 13 G-buffer channels in PtGBuffer's field order, with their float32 counts per pixel
GBUFFER_CHANNELS = (("Position", 4), ("FlatNormal", 2), ("GeometricNormal", 2), ("LinearDepth", 1), ("NormalizedDepth", 1),
                    ("MotionVector", 3), ("BaseColorMetalness", 4), ("DiffuseAlbedo", 3), ("SpecularAlbedo", 3), ("NormalRoughness", 4),
                    ("IOR", 1), ("Transmission", 1), ("Radiance", 3))
GBUFFER_WIDTH = dict(GBUFFER_CHANNELS)
# what a denoiser reads (NRD's inputs): 48 bytes per pixel against the 128 of all 13
GBUFFER_DENOISER = ("LinearDepth", "NormalRoughness", "MotionVector", "BaseColorMetalness")


class PtGBuffer(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _ in GBUFFER_CHANNELS]


# Row N27 (pt_render_gbuffer_packed, pt_render_from_gbuffer; DESIGN.md spec S30): each channel's packed texel as (numpy dtype of its raw
# words, words per pixel) -- the reference's texture formats (Source/App.cpp:431-447), 79 bytes per pixel against float32's 128 -- and the
# eight channels a frame from the G-buffer reads (Shaders/Raytracing.hlsl:118-148), in PtGBufferInput's field order
GBUFFER_PACKED = (("Position", np.float32, 4), ("FlatNormal", np.uint16, 2), ("GeometricNormal", np.uint16, 2), ("LinearDepth", np.float32, 1),
                  ("NormalizedDepth", np.float32, 1), ("MotionVector", np.uint16, 4), ("BaseColorMetalness", np.uint8, 4), ("DiffuseAlbedo", np.uint16, 4),
                  ("SpecularAlbedo", np.uint16, 4), ("NormalRoughness", np.uint16, 4), ("IOR", np.uint16, 1), ("Transmission", np.uint8, 1), ("Radiance", np.uint16, 4))
GBUFFER_PACKED_DTYPE = {name: (dtype, width) for name, dtype, width in GBUFFER_PACKED}
GBUFFER_FRAME_INPUTS = ("Position", "FlatNormal", "GeometricNormal", "BaseColorMetalness", "NormalRoughness", "IOR", "Transmission", "Radiance")
GBUFFER_FORMAT_FLOAT32, GBUFFER_FORMAT_PACKED = 0, 1


class PtGBufferPacked(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _ in GBUFFER_CHANNELS]


class PtGBufferInput(C.Structure):
    _fields_ = [("Format", C.c_uint32), ("_pad", C.c_uint32)] + [(name, C.c_void_p) for name in GBUFFER_FRAME_INPUTS]


# Row N7 (pt_render_denoiser): GraphicsSettings.Denoiser values (Source/Denoiser.ixx) and the outputs of each mode, with their float32
# counts per pixel
DENOISER_NONE, DENOISER_DLSS_RR, DENOISER_NRD_REBLUR, DENOISER_NRD_RELAX = 0, 1, 2, 3
DENOISER_OUTPUTS = {DENOISER_DLSS_RR: (("SpecularHitDistance", 1),),
                    DENOISER_NRD_REBLUR: (("Diffuse", 4), ("Specular", 4)),
                    DENOISER_NRD_RELAX: (("Diffuse", 4), ("Specular", 4))}


class PtDenoiserOutputs(C.Structure):
    _fields_ = [("Denoiser", C.c_uint32), ("_pad", C.c_uint32), ("Diffuse", C.c_void_p), ("Specular", C.c_void_p),
                ("SpecularHitDistance", C.c_void_p)]


# Row N8 (pt_nrd_composition): NRDComposition::Constants / ::Textures, and nrd::ReblurSettings().hitDistanceParameters
NRD_REBLUR_HIT_DISTANCE = (3.0, 0.1, 20.0, -25.0)
NRD_TEXTURES = ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "NoisyDiffuse", "NoisySpecular", "DenoisedDiffuse",
                "DenoisedSpecular", "Radiance")


class PtNrdCompositionConstants(C.Structure):
    _fields_ = [("RenderSize", C.c_uint32 * 2), ("Pack", C.c_uint32), ("Denoiser", C.c_uint32), ("ReBLURHitDistance", C.c_float * 4)]


class PtNrdCompositionTextures(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in NRD_TEXTURES]


# Row N9 (pt_nrd_denoise, the NRD stand-in): the settings and the nrd::ResourceType tags it reads and writes
NRD_DENOISE_TEXTURES = ("ViewZ", "MotionVector", "NormalRoughness", "BaseColorMetalness", "InDiffuse", "InSpecular", "OutDiffuse", "OutSpecular")
NRD_ACCUMULATION_CONTINUE, NRD_ACCUMULATION_RESTART, NRD_ACCUMULATION_CLEAR_AND_RESTART = 0, 1, 2


class PtNrdDenoiseSettings(C.Structure):
    _fields_ = [("RenderSize", C.c_uint32 * 2), ("Denoiser", C.c_uint32), ("AccumulationMode", C.c_uint32), ("FrameIndex", C.c_uint32),
                ("MaxDiffuseFrames", C.c_uint32), ("MaxSpecularFrames", C.c_uint32), ("AtrousIterations", C.c_uint32)]


class PtNrdDenoiseTextures(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in NRD_DENOISE_TEXTURES]


# Row N30 (pt_nrd_reblur, the ReBLUR stand-in): its settings; the buffers are PtNrdDenoiseTextures
class PtNrdReblurSettings(C.Structure):
    _fields_ = [("RenderSize", C.c_uint32 * 2), ("AccumulationMode", C.c_uint32), ("FrameIndex", C.c_uint32), ("MaxAccumulatedFrames", C.c_uint32),
                ("MaxFastAccumulatedFrames", C.c_uint32), ("HistoryFixFrames", C.c_uint32), ("MinBlurRadius", C.c_float), ("MaxBlurRadius", C.c_float),
                ("_pad", C.c_uint32 * 3)]


def nrd_reblur_settings(width, height, accumulation_mode=0, frame_index=0, max_accumulated_frames=0, max_fast_accumulated_frames=0, history_fix_frames=0,
                        min_blur_radius=0.0, max_blur_radius=0.0):
    """PtNrdReblurSettings from keywords; 0 = nrd::ReblurSettings' defaults as recollected: 30 frames, 6 fast frames, 3 history-fix frames,
    radii 1 and 30 pixels"""
    return PtNrdReblurSettings(RenderSize=(C.c_uint32 * 2)(width, height), AccumulationMode=accumulation_mode, FrameIndex=frame_index,
                               MaxAccumulatedFrames=max_accumulated_frames, MaxFastAccumulatedFrames=max_fast_accumulated_frames,
                               HistoryFixFrames=history_fix_frames, MinBlurRadius=float(min_blur_radius), MaxBlurRadius=float(max_blur_radius))


# Row N10 (pt_restir_di, the RTXDI stand-in): the settings and the buffers it reads (G-buffer channels) and writes
RESTIR_DI_INPUTS = ("Position", "GeometricNormal", "LinearDepth", "MotionVector", "BaseColorMetalness", "NormalRoughness", "IOR", "Transmission")
RESTIR_DI_TEXTURES = RESTIR_DI_INPUTS + ("Diffuse", "Specular")
RESTIR_BIAS_OFF, RESTIR_BIAS_BASIC, RESTIR_BIAS_PAIRWISE, RESTIR_BIAS_RAYTRACED = 0, 1, 2, 3


class PtRestirDiSettings(C.Structure):
    _fields_ = [("RenderSize", C.c_uint32 * 2), ("FrameIndex", C.c_uint32), ("ResetHistory", C.c_uint32), ("InitialSamples", C.c_uint32),
                ("EnableTemporal", C.c_uint32), ("TemporalBiasCorrection", C.c_uint32), ("MaxHistoryLength", C.c_uint32),
                ("EnableSpatial", C.c_uint32), ("SpatialBiasCorrection", C.c_uint32), ("SpatialSamples", C.c_uint32), ("SpatialRadius", C.c_float)]


class PtRestirDiTextures(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in RESTIR_DI_TEXTURES]


# Row N16 (pt_restir_di_sampled): the local-light sampling mode and the sizes of the presampled structures; 0 = the library's default
LIGHT_SAMPLING_UNIFORM, LIGHT_SAMPLING_POWER_RIS, LIGHT_SAMPLING_REGIR_RIS = 0, 1, 2
LIGHT_RIS_ENTRY_DTYPE = np.dtype([("light", "<u4"), ("inv_pdf", "<f4")])  # light = 0xFFFFFFFF: the entry carries nothing


class PtLightSamplingSettings(C.Structure):
    _fields_ = [("Mode", C.c_uint32), ("TileSize", C.c_uint32), ("TileCount", C.c_uint32), ("ReGIRGridSize", C.c_uint32),
                ("ReGIRLightsPerCell", C.c_uint32), ("ReGIRBuildSamples", C.c_uint32), ("ReGIRCellSize", C.c_float), ("_pad", C.c_uint32)]


def light_sampling_settings(mode=0, tile_size=0, tile_count=0, grid_size=0, lights_per_cell=0, build_samples=0, cell_size=0.0):
    return PtLightSamplingSettings(Mode=mode, TileSize=tile_size, TileCount=tile_count, ReGIRGridSize=grid_size, ReGIRLightsPerCell=lights_per_cell,
                                   ReGIRBuildSamples=build_samples, ReGIRCellSize=cell_size)


# Row N17 (pt_restir_di_ex): the BRDF candidates of initial sampling and the boiling filter; all zero = both off
class PtRestirDiCandidates(C.Structure):
    _fields_ = [("BrdfSamples", C.c_uint32), ("EnableBoilingFilter", C.c_uint32), ("BoilingFilterStrength", C.c_float), ("_pad", C.c_uint32)]


def restir_di_candidates(brdf_samples=0, boiling_filter=None):
    """boiling_filter: None / False = off, otherwise the filter's strength (the reference's defaults: brdf_samples 1, strength 0.2)"""
    on = boiling_filter is not None and boiling_filter is not False
    return PtRestirDiCandidates(BrdfSamples=brdf_samples, EnableBoilingFilter=int(on), BoilingFilterStrength=float(boiling_filter) if on else 0.0)


# Row N22 (pt_restir_di_full): final shading's reuse of a sample's visibility; the limits are literal; all zero = off
class PtRestirDiShading(C.Structure):
    _fields_ = [("ReuseFinalVisibility", C.c_uint32), ("FinalVisibilityMaxAge", C.c_uint32), ("FinalVisibilityMaxDistance", C.c_float), ("_pad", C.c_uint32)]


def restir_di_shading(reuse=False, max_age=0, max_distance=0.0):
    """the RTXDI SDK's defaults, as recollected: reuse on, max_age 4, max_distance 16"""
    return PtRestirDiShading(ReuseFinalVisibility=int(reuse), FinalVisibilityMaxAge=max_age, FinalVisibilityMaxDistance=float(max_distance))


# Row N14 (pt_render_sharc, the SHARC stand-in): SHARCSettings plus the cache's accumulation constants and the stages of a call
SHARC_UPDATE, SHARC_RESOLVE, SHARC_QUERY = 1, 2, 4
SHARC_VOXEL_DTYPE = np.dtype([("sum", "<u4", (3,)), ("w", "<u4")])  # w = samples | frames << 16 | stale << 24


class PtSharcSettings(C.Structure):
    _fields_ = [("Capacity", C.c_uint32), ("DownscaleFactor", C.c_uint32), ("SceneScale", C.c_float), ("RoughnessThreshold", C.c_float),
                ("AccumulationFrames", C.c_uint32), ("MaxStaleFrames", C.c_uint32), ("IsAntiFireflyEnabled", C.c_uint32),
                ("IsHashGridVisualizationEnabled", C.c_uint32), ("ResetHistory", C.c_uint32), ("Stages", C.c_uint32), ("_pad", C.c_uint32 * 2)]


# Row N11 (pt_upscale, the XeSS / DLSS-SR stand-in): the settings, the XeSSResourceType tags it reads and writes, and the modes of
# pt_upscale_input_size (SuperResolutionMode)
UPSCALE_TEXTURES = ("Color", "Depth", "Velocity", "Output")
UPSCALE_AUTO, UPSCALE_NATIVE, UPSCALE_QUALITY, UPSCALE_BALANCED, UPSCALE_PERFORMANCE, UPSCALE_ULTRA_PERFORMANCE = 0, 1, 2, 3, 4, 5
UPSCALE_MODES = {"auto": 0, "native": 1, "quality": 2, "balanced": 3, "performance": 4, "ultra_performance": 5}


class PtUpscaleSettings(C.Structure):
    _fields_ = [("InputSize", C.c_uint32 * 2), ("OutputSize", C.c_uint32 * 2), ("Jitter", C.c_float * 2), ("Reset", C.c_uint32),
                ("MaxHistoryWeight", C.c_float)]


class PtUpscaleTextures(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in UPSCALE_TEXTURES]


# Row N12 (pt_nis_sharpen, the NIS stand-in): sl::NISOptions' sharpness and hdrMode plus the size, and the two tagged buffers
NIS_TEXTURES = ("Color", "Output")
NIS_HDR_NONE, NIS_HDR_LINEAR, NIS_HDR_PQ = 0, 1, 2


class PtNisSettings(C.Structure):
    _fields_ = [("Size", C.c_uint32 * 2), ("Sharpness", C.c_float), ("HdrMode", C.c_uint32)]


class PtNisTextures(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in NIS_TEXTURES]


# Row N29 (pt_chromatic_aberration, spec S31): the size, the focus and the per-channel offsets, and the two buffers.  The default offsets
# are a recollection of upstream's later revision, not read from the reference tree at hand (csrc/pt_chromab.h: kCabDefaultOffsets).
CHROMATIC_ABERRATION_TEXTURES = ("Color", "Output")
CHROMATIC_ABERRATION_FOCUS_UV = (0.5, 0.5)
CHROMATIC_ABERRATION_OFFSETS = (0.003, 0.003, -0.003)
CHROMATIC_ABERRATION_MAX_OFFSET = 0.0625


class PtChromaticAberrationSettings(C.Structure):
    _fields_ = [("Size", C.c_uint32 * 2), ("FocusUV", C.c_float * 2), ("Offsets", C.c_float * 3), ("_pad", C.c_uint32)]


class PtChromaticAberrationTextures(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in CHROMATIC_ABERRATION_TEXTURES]


# Row N23 (pt_physics_*, the PhysX stand-in, spec S27): a body record, the settings, an attractor and a step's report
PHYSICS_SPRING, PHYSICS_LARGE, PHYSICS_DISABLED = 1, 2, 4
PHYSICS_INVERSE_SQUARE, PHYSICS_CONSTANT = 0, 1
PHYSICS_ALL_BODIES = 0xFFFFFFFF
PHYSICS_MAX_ATTRACTORS, PHYSICS_MAX_LARGE = 4, 64
PHYSICS_BODY_DTYPE = np.dtype([("InvMass", np.float32), ("Flags", np.uint32), ("SpringY0", np.float32), ("SpringOmega2", np.float32)])
PHYSICS_ATTRACTOR_DTYPE = np.dtype([("Body", np.uint32), ("Kind", np.uint32), ("Strength", np.float32), ("Target", np.uint32)])


class PtPhysicsSettings(C.Structure):
    _fields_ = [("Iterations", C.c_uint32), ("RebuildInterval", C.c_uint32), ("Restitution", C.c_float), ("Friction", C.c_float), ("Baumgarte", C.c_float),
                ("Slop", C.c_float), ("BounceThreshold", C.c_float), ("_pad", C.c_uint32)]


class PtPhysicsReport(C.Structure):
    _fields_ = [("Contacts", C.c_uint32), ("Clamped", C.c_uint32), ("Frozen", C.c_uint32), ("Steps", C.c_uint32)]


def physics_settings(iterations=4, rebuild_interval=0, restitution=0.6, friction=0.5, baumgarte=0.2, slop=0.005, bounce_threshold=2.0):
    """PtPhysicsSettings with S27's defaults"""
    return PtPhysicsSettings(Iterations=iterations, RebuildInterval=rebuild_interval, Restitution=restitution, Friction=friction, Baumgarte=baumgarte, Slop=slop,
                             BounceThreshold=bounce_threshold)


# Row N13 (pt_frame_gen, the DLSS-G stand-in): the sizes, the packing of the tone-mapped colour and the reset flag, and the tagged buffers
FRAME_GEN_TEXTURES = ("Color", "Depth", "MotionVector", "Output")
FRAME_GEN_RGBA8, FRAME_GEN_RGB10A2 = 0, 1


class PtFrameGenSettings(C.Structure):
    _fields_ = [("RenderSize", C.c_uint32 * 2), ("OutputSize", C.c_uint32 * 2), ("Format", C.c_uint32), ("Reset", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class PtFrameGenTextures(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in FRAME_GEN_TEXTURES]


# Row N15 (pt_ray_reconstruction, the DLSS-RR stand-in): the sizes, jitter, reset and history cap, the camera fields by value
# (Position and PtCamera.Matrices[6], [7], [2]), and the tagged buffers with their float32 counts per pixel
RAY_RECONSTRUCTION_INPUTS = (("Color", 4), ("Depth", 1), ("MotionVector", 3), ("NormalRoughness", 4), ("DiffuseAlbedo", 3), ("SpecularAlbedo", 3),
                             ("SpecularHitDistance", 1))
RAY_RECONSTRUCTION_TEXTURES = tuple(name for name, _ in RAY_RECONSTRUCTION_INPUTS) + ("Output",)
CAMERA_PREVIOUS_WORLD_TO_PROJECTION, CAMERA_PROJECTION_TO_VIEW, CAMERA_VIEW_TO_WORLD = 2, 6, 7  # indices into PtCamera.Matrices


class PtRayReconstructionSettings(C.Structure):
    _fields_ = [("RenderSize", C.c_uint32 * 2), ("OutputSize", C.c_uint32 * 2), ("Jitter", C.c_float * 2), ("Reset", C.c_uint32),
                ("MaxHistoryWeight", C.c_float), ("Position", C.c_float * 3), ("_pad", C.c_float), ("ProjectionToView", C.c_float * 16),
                ("ViewToWorld", C.c_float * 16), ("PreviousWorldToProjection", C.c_float * 16)]


class PtRayReconstructionTextures(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in RAY_RECONSTRUCTION_TEXTURES]


def ray_reconstruction_settings(render_size, output_size, camera, jitter=None, reset=False, max_history_weight=0.0):
    """PtRayReconstructionSettings from a PtCamera: its Position and three matrices by value; jitter defaults to -camera.Jitter, what
    the reference hands its upscalers"""
    s = PtRayReconstructionSettings(RenderSize=(C.c_uint32 * 2)(*render_size), OutputSize=(C.c_uint32 * 2)(*output_size), Reset=1 if reset else 0,
                                    MaxHistoryWeight=max_history_weight)
    jitter = (-camera.Jitter[0], -camera.Jitter[1]) if jitter is None else jitter
    s.Jitter[0], s.Jitter[1] = jitter
    for k in range(3):
        s.Position[k] = camera.Position[k]
    for k in range(16):
        s.ProjectionToView[k] = camera.Matrices[CAMERA_PROJECTION_TO_VIEW][k]
        s.ViewToWorld[k] = camera.Matrices[CAMERA_VIEW_TO_WORLD][k]
        s.PreviousWorldToProjection[k] = camera.Matrices[CAMERA_PREVIOUS_WORLD_TO_PROJECTION][k]
    return s


# pt_render_with_di: the frame's direct illumination, supplied by the caller (device pointers, float4 per pixel of the rect)
class PtDirectLighting(C.Structure):
    _fields_ = [("Diffuse", C.c_void_p), ("Specular", C.c_void_p)]


class PtTextureMapInfo(C.Structure):
    _fields_ = [("Descriptor", C.c_uint32), ("TextureCoordinateIndex", C.c_uint32), ("_pad", C.c_uint32 * 2)]


TEXTURE_MAP_BASE_COLOR, TEXTURE_MAP_EMISSIVE_COLOR, TEXTURE_MAP_METALLIC, TEXTURE_MAP_ROUGHNESS = 0, 1, 2, 3
TEXTURE_MAP_METALLIC_ROUGHNESS, TEXTURE_MAP_TRANSMISSION, TEXTURE_MAP_NORMAL, TEXTURE_MAP_COUNT = 4, 5, 6, 7
TEXTURE_RGBA8_UNORM, TEXTURE_RGBA8_UNORM_SRGB, TEXTURE_RGBA32_FLOAT = 0, 1, 2


class PtObjectTextures(C.Structure):
    _fields_ = [("Maps", PtTextureMapInfo * TEXTURE_MAP_COUNT)]


class PtTexture(C.Structure):
    _fields_ = [("Pixels", C.c_void_p), ("Width", C.c_uint32), ("Height", C.c_uint32), ("Format", C.c_uint32), ("_pad", C.c_uint32)]


class PtToneMapParams(C.Structure):
    _fields_ = [("Operator", C.c_uint32), ("TransferFunction", C.c_uint32), ("LinearExposure", C.c_float), ("PaperWhiteNits", C.c_float),
                ("ColorRotation", C.c_uint32), ("_pad", C.c_uint32 * 3)]


TONE_NONE, TONE_SATURATE, TONE_REINHARD, TONE_ACES_FILMIC = 0, 1, 2, 3          # DirectX::ToneMapPostProcess::Operator
TRANSFER_LINEAR, TRANSFER_SRGB, TRANSFER_ST2084 = 0, 1, 2                       # ::TransferFunction
ROTATE_709_TO_2020, ROTATE_P3D65_TO_2020, ROTATE_709_TO_P3D65 = 0, 1, 2          # ::ColorPrimaryRotation


def tonemap_params(operator=TONE_ACES_FILMIC, transfer=TRANSFER_SRGB, exposure_stops=0.0, paper_white_nits=200.0, rotation=ROTATE_709_TO_2020):
    """the reference's defaults (Source/MyAppData.h:313-330): ACESFilmic + sRGB at exposure 0 for SDR, 200 nits / HDTV_to_UHDTV for HDR10"""
    p = PtToneMapParams()
    p.Operator, p.TransferFunction, p.ColorRotation = operator, transfer, rotation
    p.LinearExposure = 2.0 ** exposure_stops  # SetExposure: linear exposure = 2^stops
    p.PaperWhiteNits = paper_white_nits
    return p


class PtConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("tile_size", C.c_uint32), ("stream", C.c_uint64), ("flags", C.c_uint32), ("frames_in_flight", C.c_uint32)]


class PtAccelInfo(C.Structure):
    _fields_ = [
        ("leaf_count", C.c_uint32), ("node_count", C.c_uint32), ("depth", C.c_uint32), ("lds_resident", C.c_uint32),
        ("bounds_min", C.c_float * 3), ("bounds_max", C.c_float * 3), ("build_ms", C.c_float), ("builder", C.c_uint32),
    ]


class PtStats(C.Structure):
    _fields_ = [
        ("rays", C.c_uint64), ("paths", C.c_uint64), ("pixels", C.c_uint64), ("ms_total", C.c_double),
        ("ms_traverse", C.c_double), ("ms_shade", C.c_double), ("traverse_launches", C.c_uint32),
        ("shade_launches", C.c_uint32), ("bytes_algorithmic", C.c_uint64),
        ("ms_tail", C.c_double), ("tail_launches", C.c_uint32), ("beams_used", C.c_uint32),
        ("rays_first_pass_inline", C.c_uint64), ("node_visits", C.c_uint64), ("sphere_tests", C.c_uint64),
    ]


class PtBvhNode(C.Structure):
    _fields_ = [
        ("lo0", C.c_float * 3), ("hi0", C.c_float * 3), ("lo1", C.c_float * 3), ("hi1", C.c_float * 3),
        ("child0", C.c_int32), ("child1", C.c_int32), ("parent", C.c_int32), ("_pad", C.c_int32),
    ]


assert C.sizeof(PtSphere) == 16 and C.sizeof(PtMaterial) == 64 and C.sizeof(PtCamera) == 608
assert C.sizeof(PtSceneData) == 80 and C.sizeof(PtGraphicsSettings) == 80 and C.sizeof(PtBvhNode) == 64
assert C.sizeof(PtRayReconstructionSettings) == 240 and PtRayReconstructionSettings.PreviousWorldToProjection.offset == 176

SPHERE_DTYPE = np.dtype([("cx", "<f4"), ("cy", "<f4"), ("cz", "<f4"), ("r", "<f4")])
MATERIAL_DTYPE = np.dtype([
    ("BaseColor", "<f4", (4,)), ("EmissiveStrength", "<f4"), ("EmissiveColor", "<f4", (3,)), ("Metallic", "<f4"),
    ("Roughness", "<f4"), ("IOR", "<f4"), ("Transmission", "<f4"), ("AlphaMode", "<u4"), ("AlphaCutoff", "<f4"), ("_pad", "<u4", (2,)),
])
BVH_NODE_DTYPE = np.dtype([
    ("lo0", "<f4", (3,)), ("hi0", "<f4", (3,)), ("lo1", "<f4", (3,)), ("hi1", "<f4", (3,)),
    ("child0", "<i4"), ("child1", "<i4"), ("parent", "<i4"), ("_pad", "<i4"),
])
assert SPHERE_DTYPE.itemsize == 16 and MATERIAL_DTYPE.itemsize == 64 and BVH_NODE_DTYPE.itemsize == 64

PT_FLAG_NO_LDS_SCENE = 1
PT_FLAG_NO_GRAPH = 2
PT_FLAG_HOST_LBVH = 4
PT_FLAG_SPLIT_KERNELS = 8
PT_FLAG_TWO_FRAMES_IN_FLIGHT = 16
PT_FLAG_DEFAULT_STREAM = 32
PT_FLAG_FAST_BUILD = 64
PT_BUILDER_DEVICE_LBVH, PT_BUILDER_HOST_LBVH, PT_BUILDER_HOST_SAH = 0, 1, 2


def default_material(n=1):
    """Material defaults of Source/Material.ixx:13-18."""
    m = np.zeros(n, dtype=MATERIAL_DTYPE)
    m["BaseColor"] = (0, 0, 0, 1)
    m["EmissiveStrength"] = 1
    m["Roughness"] = 0.5
    m["IOR"] = 1.5
    m["AlphaCutoff"] = 0.5
    return m


def graphics_settings(width, height, frame_index=0, bounces=8, spp=1, rr=True, threshold=1e-3, di=False):
    """GraphicsSettings with the reference defaults that carry over; di = IsDIEnabled (row N4)."""
    gs = PtGraphicsSettings()
    gs.RenderSize[0], gs.RenderSize[1] = width, height
    gs.FrameIndex, gs.Bounces, gs.SamplesPerPixel = frame_index, bounces, spp
    gs.ThroughputThreshold = threshold
    gs.IsRussianRouletteEnabled = 1 if rr else 0
    gs.IsDIEnabled = 1 if di else 0
    return gs
