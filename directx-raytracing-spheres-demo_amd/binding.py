"""ctypes binding of the C-ABI (include/pt_api.h) exported by libpt_hip.so, plus a thin ``Renderer`` convenience
class shaped like the reference's pass object (Raytracing::SetConstants / Render, Source/Raytracing.ixx:92-112).

No CPU fallback: if the library is absent or there is no GPU, construction raises."""
import ctypes as C
import os

import numpy as np

from .abi_types import (BVH_NODE_DTYPE, DENOISER_OUTPUTS, FRAME_GEN_TEXTURES, GBUFFER_CHANNELS, GBUFFER_FRAME_INPUTS, GBUFFER_PACKED_DTYPE, PtGBufferInput, PtGBufferPacked, NIS_TEXTURES, NRD_DENOISE_TEXTURES, NRD_REBLUR_HIT_DISTANCE, NRD_TEXTURES, PtAccelInfo,
                        PtCamera, PtConfig, PtDenoiserOutputs, PtDirectLighting, PtFrameGenSettings, PtFrameGenTextures, PtGBuffer, PtGraphicsSettings, PtNisSettings, PtNisTextures, PtChromaticAberrationSettings, PtChromaticAberrationTextures, CHROMATIC_ABERRATION_TEXTURES, CHROMATIC_ABERRATION_FOCUS_UV, CHROMATIC_ABERRATION_OFFSETS, PtNrdCompositionConstants, PtNrdCompositionTextures,
                        PtNrdDenoiseSettings, PtNrdDenoiseTextures, PtNrdReblurSettings, nrd_reblur_settings, PtRect, PtLightSamplingSettings, LIGHT_RIS_ENTRY_DTYPE, light_sampling_settings, PtRestirDiCandidates, restir_di_candidates, PtRestirDiShading, restir_di_shading, PtRestirDiSettings, PtSharcSettings, PtRestirDiTextures, PtSceneData, PtStats, PtUpscaleSettings, PtUpscaleTextures,
                        PtRayReconstructionSettings, PtRayReconstructionTextures, RAY_RECONSTRUCTION_TEXTURES, RESTIR_DI_TEXTURES, UPSCALE_TEXTURES,
                        ray_reconstruction_settings, PHYSICS_ATTRACTOR_DTYPE, PHYSICS_BODY_DTYPE, PtPhysicsReport, PtPhysicsSettings, physics_settings)

_PKG = os.path.dirname(os.path.abspath(__file__))

STATUS = {0: "PT_OK", 1: "PT_ERR_INVALID_ARG", 2: "PT_ERR_NO_DEVICE", 3: "PT_ERR_HIP", 4: "PT_ERR_STATE", 5: "PT_ERR_UNSUPPORTED", 6: "PT_ERR_OOM"}

# every symbol include/pt_api.h declares
API_SYMBOLS = [
    "pt_create", "pt_destroy", "pt_set_scene", "pt_build_accel", "pt_update_spheres", "pt_refit_accel", "pt_set_camera", "pt_set_constants", "pt_render",
    "pt_set_partition", "pt_tiles_count", "pt_render_tiles", "pt_unpack_tiles", "pt_set_partition_ex", "pt_tiles_count_ex", "pt_unpack_tiles_ex", "pt_tonemap", "pt_accumulate", "pt_bloom", "pt_render_gbuffer", "pt_render_denoiser", "pt_render_with_di", "pt_nrd_composition", "pt_nrd_denoise", "pt_nrd_reblur", "pt_nrd_reblur_history", "pt_restir_di", "pt_restir_di_sampled", "pt_restir_di_ex", "pt_restir_di_full", "pt_restir_di_history", "pt_light_ris_download", "pt_render_sharc", "pt_render_sharc_ex", "pt_sharc_download", "pt_sharc_upload", "pt_render_lens", "pt_render_gbuffer_packed", "pt_render_from_gbuffer", "pt_upscale", "pt_upscale_input_size", "pt_nis_sharpen", "pt_chromatic_aberration", "pt_frame_gen", "pt_ray_reconstruction", "pt_ray_reconstruction_history", "pt_set_textures", "pt_update_rotations", "pt_pack_rgb", "pt_unpack_tiles_rgb", "pt_trace_rays", "pt_trace_rays_stats", "pt_accel_download",
    "pt_accel_download_order", "pt_accel_download_wide", "pt_lbvh_build_host", "pt_sah_build_host", "pt_set_profiling", "pt_get_profile", "pt_get_totals", "pt_get_queue_sizes", "pt_get_refl_stats", "pt_synchronize", "pt_last_error", "pt_version",
    "pt_comm_unique_id", "pt_comm_init", "pt_comm_destroy", "pt_gather", "pt_device_alloc", "pt_device_free", "pt_download",
    "pt_physics_create", "pt_physics_set_attractors", "pt_physics_step", "pt_physics_download", "pt_physics_destroy",
    "pt_physics_publish", "pt_render_gbuffer_published",
]


class PtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS.get(status, status)}: {message}")
        self.status = status


def hip_library_path():
    # PT_HIP_LIB: another build of the same library (A/B runs of kernel variants on one box: tools/experiments)
    return os.environ.get("PT_HIP_LIB") or os.path.join(_PKG, "libpt_hip.so")


class HipLib:
    def __init__(self, path=None):
        path = path or hip_library_path()
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not built: the HIP extension is required (no CPU fallback)")
        self.lib = lib = C.CDLL(path)
        vp, u32 = C.c_void_p, C.c_uint32
        lib.pt_create.restype = C.c_int
        lib.pt_create.argtypes = [C.POINTER(PtConfig), C.POINTER(vp)]
        lib.pt_destroy.restype = None
        lib.pt_destroy.argtypes = [vp]
        lib.pt_set_scene.restype = C.c_int
        lib.pt_set_scene.argtypes = [vp, vp, vp, u32, C.POINTER(PtSceneData)]
        lib.pt_build_accel.restype = C.c_int
        lib.pt_build_accel.argtypes = [vp, C.POINTER(PtAccelInfo)]
        lib.pt_update_spheres.restype = C.c_int
        lib.pt_update_spheres.argtypes = [vp, vp, u32]
        lib.pt_refit_accel.restype = C.c_int
        lib.pt_refit_accel.argtypes = [vp]
        lib.pt_set_camera.restype = C.c_int
        lib.pt_set_camera.argtypes = [vp, C.POINTER(PtCamera)]
        lib.pt_set_constants.restype = C.c_int
        lib.pt_set_constants.argtypes = [vp, C.POINTER(PtGraphicsSettings)]
        lib.pt_render.restype = C.c_int
        lib.pt_render.argtypes = [vp, C.POINTER(PtRect), vp, C.c_int, C.POINTER(PtStats)]
        lib.pt_set_partition.restype = C.c_int
        lib.pt_set_partition.argtypes = [vp, u32, u32]
        lib.pt_tiles_count.restype = u32
        lib.pt_tiles_count.argtypes = [vp, u32]
        lib.pt_render_tiles.restype = C.c_int
        lib.pt_render_tiles.argtypes = [vp, vp, C.POINTER(PtStats)]
        lib.pt_unpack_tiles.restype = C.c_int
        lib.pt_unpack_tiles.argtypes = [vp, vp, u32, vp]
        lib.pt_set_partition_ex.restype = C.c_int
        lib.pt_set_partition_ex.argtypes = [vp, u32, u32, u32]
        lib.pt_tiles_count_ex.restype = u32
        lib.pt_tiles_count_ex.argtypes = [vp, u32, u32, u32]
        lib.pt_unpack_tiles_ex.restype = C.c_int
        lib.pt_unpack_tiles_ex.argtypes = [vp, vp, C.c_uint64, u32, u32, u32, u32, vp]
        lib.pt_pack_rgb.restype = C.c_int
        lib.pt_pack_rgb.argtypes = [vp, vp, C.c_uint64, vp]
        lib.pt_unpack_tiles_rgb.restype = C.c_int
        lib.pt_unpack_tiles_rgb.argtypes = [vp, vp, C.c_uint64, u32, u32, u32, u32, vp]
        lib.pt_set_textures.restype = C.c_int
        lib.pt_set_textures.argtypes = [vp, vp, u32, vp, vp]
        lib.pt_update_rotations.restype = C.c_int
        lib.pt_update_rotations.argtypes = [vp, vp, u32]
        lib.pt_tonemap.restype = C.c_int
        lib.pt_tonemap.argtypes = [vp, vp, u32, vp, vp]
        lib.pt_accumulate.restype = C.c_int
        lib.pt_accumulate.argtypes = [vp, vp, vp, u32, u32]
        lib.pt_bloom.restype = C.c_int
        lib.pt_bloom.argtypes = [vp, vp, vp, u32, u32, C.c_float]
        lib.pt_render_gbuffer.restype = C.c_int
        lib.pt_render_gbuffer.argtypes = [vp, C.POINTER(PtRect), C.POINTER(PtGBuffer), vp, vp]
        lib.pt_render_denoiser.restype = C.c_int
        lib.pt_render_denoiser.argtypes = [vp, C.POINTER(PtRect), vp, C.c_int, C.POINTER(PtDenoiserOutputs), C.POINTER(PtStats)]
        lib.pt_render_with_di.restype = C.c_int
        lib.pt_render_with_di.argtypes = [vp, C.POINTER(PtRect), vp, C.c_int, C.POINTER(PtDirectLighting), C.POINTER(PtDenoiserOutputs), C.POINTER(PtStats)]
        lib.pt_nrd_composition.restype = C.c_int
        lib.pt_nrd_composition.argtypes = [vp, C.POINTER(PtNrdCompositionConstants), C.POINTER(PtNrdCompositionTextures)]
        lib.pt_nrd_denoise.restype = C.c_int
        lib.pt_nrd_denoise.argtypes = [vp, C.POINTER(PtNrdDenoiseSettings), C.POINTER(PtNrdDenoiseTextures)]
        lib.pt_nrd_reblur.restype = C.c_int
        lib.pt_nrd_reblur.argtypes = [vp, C.POINTER(PtNrdReblurSettings), C.POINTER(PtNrdDenoiseTextures)]
        lib.pt_nrd_reblur_history.restype = C.c_int
        lib.pt_nrd_reblur_history.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.pt_restir_di.restype = C.c_int
        lib.pt_restir_di.argtypes = [vp, C.POINTER(PtRestirDiSettings), C.POINTER(PtRestirDiTextures)]
        lib.pt_restir_di_sampled.restype = C.c_int
        lib.pt_restir_di_sampled.argtypes = [vp, C.POINTER(PtRestirDiSettings), C.POINTER(PtLightSamplingSettings), C.POINTER(PtRestirDiTextures)]
        lib.pt_restir_di_ex.restype = C.c_int
        lib.pt_restir_di_ex.argtypes = [vp, C.POINTER(PtRestirDiSettings), C.POINTER(PtLightSamplingSettings), C.POINTER(PtRestirDiCandidates), C.POINTER(PtRestirDiTextures)]
        lib.pt_restir_di_full.restype = C.c_int
        lib.pt_restir_di_full.argtypes = [vp, C.POINTER(PtRestirDiSettings), C.POINTER(PtLightSamplingSettings), C.POINTER(PtRestirDiCandidates), C.POINTER(PtRestirDiShading),
                                          C.POINTER(PtRestirDiTextures)]
        lib.pt_restir_di_history.restype = C.c_int
        lib.pt_restir_di_history.argtypes = [vp, u32, vp, vp]
        lib.pt_light_ris_download.restype = C.c_int
        lib.pt_light_ris_download.argtypes = [vp, vp, C.POINTER(u32), vp, C.POINTER(u32)]
        lib.pt_render_sharc.restype = C.c_int
        lib.pt_render_sharc.argtypes = [vp, C.POINTER(PtRect), vp, C.c_int, C.POINTER(PtSharcSettings), C.POINTER(PtStats)]
        lib.pt_render_sharc_ex.restype = C.c_int
        lib.pt_render_sharc_ex.argtypes = [vp, C.POINTER(PtRect), vp, C.c_int, C.POINTER(PtSharcSettings), C.POINTER(PtDirectLighting), C.POINTER(PtDenoiserOutputs),
                                           C.POINTER(PtStats)]
        lib.pt_sharc_download.restype = C.c_int
        lib.pt_sharc_download.argtypes = [vp, vp, vp, u32]
        lib.pt_sharc_upload.restype = C.c_int
        lib.pt_sharc_upload.argtypes = [vp, vp, vp, u32]
        lib.pt_render_lens.restype = C.c_int
        lib.pt_render_lens.argtypes = [vp, C.POINTER(PtRect), vp, C.c_int, C.POINTER(PtStats)]
        lib.pt_render_gbuffer_packed.restype = C.c_int
        lib.pt_render_gbuffer_packed.argtypes = [vp, C.POINTER(PtRect), C.POINTER(PtGBufferPacked), vp, vp]
        lib.pt_render_from_gbuffer.restype = C.c_int
        lib.pt_render_from_gbuffer.argtypes = [vp, C.POINTER(PtRect), vp, C.c_int, C.POINTER(PtGBufferInput), C.POINTER(PtDirectLighting), C.POINTER(PtStats)]
        lib.pt_upscale.restype = C.c_int
        lib.pt_upscale.argtypes = [vp, C.POINTER(PtUpscaleSettings), C.POINTER(PtUpscaleTextures)]
        lib.pt_upscale_input_size.restype = C.c_int
        lib.pt_upscale_input_size.argtypes = [u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
        lib.pt_nis_sharpen.restype = C.c_int
        lib.pt_nis_sharpen.argtypes = [vp, C.POINTER(PtNisSettings), C.POINTER(PtNisTextures)]
        lib.pt_chromatic_aberration.restype = C.c_int
        lib.pt_chromatic_aberration.argtypes = [vp, C.POINTER(PtChromaticAberrationSettings), C.POINTER(PtChromaticAberrationTextures)]
        lib.pt_frame_gen.restype = C.c_int
        lib.pt_frame_gen.argtypes = [vp, C.POINTER(PtFrameGenSettings), C.POINTER(PtFrameGenTextures), C.POINTER(u32)]
        lib.pt_ray_reconstruction.restype = C.c_int
        lib.pt_ray_reconstruction.argtypes = [vp, C.POINTER(PtRayReconstructionSettings), C.POINTER(PtRayReconstructionTextures)]
        lib.pt_ray_reconstruction_history.restype = C.c_int
        lib.pt_ray_reconstruction_history.argtypes = [vp, vp, vp, vp]
        lib.pt_trace_rays.restype = C.c_int
        lib.pt_trace_rays.argtypes = [vp, vp, vp, u32, C.c_float, C.c_int, vp, vp]
        lib.pt_trace_rays_stats.restype = C.c_int
        lib.pt_trace_rays_stats.argtypes = [vp, vp, vp, u32, C.c_float, vp, vp, vp]
        lib.pt_accel_download.restype = C.c_int
        lib.pt_accel_download.argtypes = [vp, vp, u32]
        lib.pt_accel_download_order.restype = C.c_int
        lib.pt_accel_download_order.argtypes = [vp, vp, u32]
        lib.pt_accel_download_wide.restype = C.c_int
        lib.pt_accel_download_wide.argtypes = [vp, vp, u32, C.POINTER(u32)]
        lib.pt_lbvh_build_host.restype = C.c_int
        lib.pt_lbvh_build_host.argtypes = [vp, u32, vp, vp, C.POINTER(u32)]
        lib.pt_sah_build_host.restype = C.c_int
        lib.pt_sah_build_host.argtypes = [vp, u32, vp, vp, C.POINTER(u32)]
        lib.pt_set_profiling.restype = C.c_int
        lib.pt_set_profiling.argtypes = [vp, C.c_int]
        lib.pt_get_profile.restype = C.c_int
        lib.pt_get_profile.argtypes = [vp, C.POINTER(PtStats), C.c_int]
        lib.pt_get_totals.restype = C.c_int
        lib.pt_get_totals.argtypes = [vp, C.POINTER(PtStats), C.c_int]
        lib.pt_get_refl_stats.restype = C.c_int
        lib.pt_get_refl_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
        lib.pt_get_queue_sizes.restype = C.c_int
        lib.pt_get_queue_sizes.argtypes = [vp, vp, u32, C.POINTER(u32)]
        lib.pt_physics_create.restype = C.c_int
        lib.pt_physics_create.argtypes = [vp, vp, vp, vp, vp, vp, u32, C.POINTER(PtPhysicsSettings)]
        lib.pt_physics_set_attractors.restype = C.c_int
        lib.pt_physics_set_attractors.argtypes = [vp, vp, u32]
        lib.pt_physics_step.restype = C.c_int
        lib.pt_physics_step.argtypes = [vp, C.c_float, u32, C.POINTER(PtPhysicsReport)]
        lib.pt_physics_download.restype = C.c_int
        lib.pt_physics_download.argtypes = [vp, vp, vp, vp, vp]
        lib.pt_physics_destroy.restype = None
        lib.pt_physics_destroy.argtypes = [vp]
        lib.pt_physics_publish.restype = C.c_int
        lib.pt_physics_publish.argtypes = [vp]
        lib.pt_render_gbuffer_published.restype = C.c_int
        lib.pt_render_gbuffer_published.argtypes = [vp, C.POINTER(PtRect), C.POINTER(PtGBuffer)]
        lib.pt_synchronize.restype = C.c_int
        lib.pt_synchronize.argtypes = [vp]
        lib.pt_comm_unique_id.restype = C.c_int
        lib.pt_comm_unique_id.argtypes = [vp]
        lib.pt_comm_init.restype = C.c_int
        lib.pt_comm_init.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
        lib.pt_comm_destroy.restype = C.c_int
        lib.pt_comm_destroy.argtypes = [vp]
        lib.pt_gather.restype = C.c_int
        lib.pt_gather.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32]
        lib.pt_last_error.restype = C.c_char_p
        lib.pt_last_error.argtypes = [vp]
        lib.pt_version.restype = C.c_char_p
        lib.pt_version.argtypes = []


    def upscale_input_size(self, mode, out_w, out_h):
        """pt_upscale_input_size (no GPU needed): the RenderSize of a super-resolution mode (abi_types.UPSCALE_*) for an output size"""
        w, h = C.c_uint32(0), C.c_uint32(0)
        st = self.lib.pt_upscale_input_size(mode, out_w, out_h, C.byref(w), C.byref(h))
        if st != 0:
            raise PtError(st, "pt_upscale_input_size")
        return w.value, h.value

    def lbvh_build_host(self, spheres, sah=False):
        """Host LBVH builder, or with sah=True the host SAH builder of small scenes (no GPU needed)
        -> (nodes[BVH_NODE_DTYPE], sorted_id, depth)."""
        spheres = np.ascontiguousarray(spheres)
        n = len(spheres)
        nodes = np.zeros(max(n - 1, 0), dtype=BVH_NODE_DTYPE)
        order = np.zeros(n, dtype=np.uint32)
        depth = C.c_uint32(0)
        fn = self.lib.pt_sah_build_host if sah else self.lib.pt_lbvh_build_host
        st = fn(spheres.ctypes.data, n, nodes.ctypes.data if n > 1 else None, order.ctypes.data, C.byref(depth))
        if st != 0:
            raise PtError(st, "pt_lbvh_build_host")
        return nodes, order, depth.value


_hip = None


def load_hip():
    """Load libpt_hip.so once.  If torch is already imported, let it initialise its (bundled) ROCm runtime first:
    loading /opt/rocm's runtime before torch's makes torch report "No HIP GPUs are available" later."""
    global _hip
    if _hip is None:
        import sys

        torch = sys.modules.get("torch")
        if torch is not None:
            try:
                if torch.cuda.is_available():
                    torch.cuda.init()
            except Exception:
                pass
        _hip = HipLib()
    return _hip


class Renderer:
    """One PtContext.  Methods mirror the C-ABI one to one; errors raise PtError with pt_last_error()."""

    def __init__(self, device=0, flags=0, stream=0, tile_size=0, lib=None, frames_in_flight=0):
        self._lib = (lib or load_hip()).lib
        cfg = PtConfig(device=device, tile_size=tile_size, stream=stream, flags=flags, frames_in_flight=frames_in_flight)
        ctx = C.c_void_p()
        st = self._lib.pt_create(C.byref(cfg), C.byref(ctx))
        if st != 0:
            raise PtError(st, "pt_create failed (a HIP device is required; there is no CPU fallback)")
        self._ctx = ctx
        self.accel = None
        self._gs = None

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.pt_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise PtError(st, self._lib.pt_last_error(self._ctx).decode())

    def set_scene(self, spheres, materials, scene_data, build=True):
        spheres = np.ascontiguousarray(spheres)
        materials = np.ascontiguousarray(materials)
        assert spheres.dtype.itemsize == 16 and materials.dtype.itemsize == 64 and len(spheres) == len(materials)
        self._check(self._lib.pt_set_scene(self._ctx, spheres.ctypes.data, materials.ctypes.data, len(spheres), C.byref(scene_data)))
        return self.build_accel() if build else None

    def build_accel(self):
        info = PtAccelInfo()
        self._check(self._lib.pt_build_accel(self._ctx, C.byref(info)))
        self.accel = info
        return info

    def update_spheres(self, spheres, refit=True):
        """New centres / radii for the same objects, applied to the next frame (asynchronous); refit the LBVH boxes."""
        spheres = np.ascontiguousarray(spheres)
        assert spheres.dtype.itemsize == 16
        self._check(self._lib.pt_update_spheres(self._ctx, spheres.ctypes.data, len(spheres)))
        if refit:
            self._check(self._lib.pt_refit_accel(self._ctx))

    def set_camera(self, camera):
        self._check(self._lib.pt_set_camera(self._ctx, C.byref(camera)))

    def set_constants(self, gs):
        self._check(self._lib.pt_set_constants(self._ctx, C.byref(gs)))
        self._gs = gs

    def set_partition(self, rank, world):
        self._check(self._lib.pt_set_partition(self._ctx, rank, world))

    def tiles_count(self, rank):
        return int(self._lib.pt_tiles_count(self._ctx, rank))

    def set_partition_ex(self, first, run, stride):
        """own the tiles t with first <= t % stride < first + run (weighted partition; see include/pt_api.h)"""
        self._check(self._lib.pt_set_partition_ex(self._ctx, first, run, stride))

    def tiles_count_ex(self, first, run, stride):
        return int(self._lib.pt_tiles_count_ex(self._ctx, first, run, stride))

    def set_profiling(self, enabled):
        self._check(self._lib.pt_set_profiling(self._ctx, 1 if enabled else 0))

    def profile(self, reset=False):
        """Summed per-launch event times over every render call since profiling was switched on (synchronises)."""
        stats = PtStats()
        self._check(self._lib.pt_get_profile(self._ctx, C.byref(stats), 1 if reset else 0))
        return stats

    def totals(self, reset=False):
        """Device-accumulated totals over all render calls since the last reset (synchronises)."""
        stats = PtStats()
        self._check(self._lib.pt_get_totals(self._ctx, C.byref(stats), 1 if reset else 0))
        return stats

    def refl_stats(self, reset=False):
        """Reflection beams: (waves that traced in-register bounce-1 rays, ... of them served by a region list) since the last reset."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.pt_get_refl_stats(self._ctx, C.byref(a), C.byref(b), 1 if reset else 0))
        return a.value, b.value

    def queue_sizes(self):
        """Ray-queue sizes of the last spp == 1 frame: [slots, rays at bounce 1, rays at bounce 2, ...]."""
        buf = np.zeros(256, dtype=np.uint32)
        n = C.c_uint32(0)
        self._check(self._lib.pt_get_queue_sizes(self._ctx, buf.ctypes.data, len(buf), C.byref(n)))
        return [int(x) for x in buf[: n.value]]

    # ---- pt_physics_* (row N23, spec S27): the rigid-sphere state the context owns
    def physics_create(self, spheres, bodies, lin_vel=None, ang_vel=None, rotations=None, settings=None):
        """spheres: (n, 4) float32 or the PtSphere dtype; bodies: PHYSICS_BODY_DTYPE; velocities (n, 3), rotations (n, 4) or None (zero,
        identity); settings: PtPhysicsSettings or None (S27's defaults).  Replaces any earlier state; builds the tree (synchronous)."""
        spheres = np.ascontiguousarray(spheres)
        assert spheres.dtype.itemsize * (spheres.shape[-1] if spheres.ndim > 1 else 1) == 16
        bodies = np.ascontiguousarray(bodies, dtype=PHYSICS_BODY_DTYPE)
        n = len(spheres)
        assert len(bodies) == n
        opt = [None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(n, k) for a, k in ((lin_vel, 3), (ang_vel, 3), (rotations, 4))]
        self._check(self._lib.pt_physics_create(self._ctx, spheres.ctypes.data if n else None, bodies.ctypes.data if n else None,
                                                *[None if a is None or n == 0 else a.ctypes.data for a in opt], n, C.byref(settings) if settings is not None else None))
        self._physics_n = n

    def physics_set_attractors(self, attractors):
        """attractors: PHYSICS_ATTRACTOR_DTYPE records, or (Body, Kind, Strength, Target) tuples; at most 4"""
        a = np.array([tuple(x) for x in attractors], dtype=PHYSICS_ATTRACTOR_DTYPE)
        self._check(self._lib.pt_physics_set_attractors(self._ctx, a.ctypes.data if len(a) else None, len(a)))

    def physics_step(self, dt, substeps=1, report=True):
        """`substeps` steps of dt / substeps on the context's stream -> PtPhysicsReport (waits), or None with report=False (asynchronous)"""
        r = PtPhysicsReport() if report else None
        self._check(self._lib.pt_physics_step(self._ctx, dt, substeps, C.byref(r) if report else None))
        return r

    def physics_download(self, spheres=True, rotations=True, lin_vel=True, ang_vel=True):
        """-> (spheres (n, 4), rotations (n, 4), lin_vel (n, 3), ang_vel (n, 3)); None for what was not asked for.  Waits for the stream."""
        n = self._physics_n
        out = [np.zeros((n, k), np.float32) if want else None for want, k in ((spheres, 4), (rotations, 4), (lin_vel, 3), (ang_vel, 3))]
        self._check(self._lib.pt_physics_download(self._ctx, *[None if a is None else a.ctypes.data for a in out]))
        return tuple(out)

    def physics_destroy(self):
        self._lib.pt_physics_destroy(self._ctx)

    def physics_publish(self):
        """Row N24 (spec S28): the simulation's current pose becomes the pose of every frame from the next render call on -- what
        physics_download + update_spheres (+ update_rotations with textures) do, on the device: asynchronous on the context's stream,
        no refit call needed."""
        self._check(self._lib.pt_physics_publish(self._ctx))

    def synchronize(self):
        self._check(self._lib.pt_synchronize(self._ctx))

    # ---- multi-GPU exchange (pt_comm_* / pt_gather): RCCL behind the C-ABI
    def comm_unique_id(self):
        """128-byte communicator id (rank 0 makes it and ships it to the other ranks)"""
        buf = (C.c_ubyte * 128)()
        st = self._lib.pt_comm_unique_id(buf)
        if st != 0:
            raise PtError(st, "pt_comm_unique_id: RCCL could not be loaded" if st == 5 else "pt_comm_unique_id")
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self._check(self._lib.pt_comm_init(self._ctx, buf, rank, world))

    def comm_destroy(self):
        self._check(self._lib.pt_comm_destroy(self._ctx))

    def gather(self, send_ptr, recv_ptr, nbytes, root=0):
        """every rank but `root` sends nbytes from send_ptr; the root receives world - 1 parts into recv_ptr (device pointers)"""
        self._check(self._lib.pt_gather(self._ctx, C.c_void_p(send_ptr or 0), C.c_void_p(recv_ptr or 0), int(nbytes), int(root)))

    def render(self, rect=None, want_stats=True):
        """Render to a host numpy array (h, w, 4) float32.  rect = (x, y, w, h) or None for the full frame."""
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        r = PtRect(*rect)
        out = np.empty((r.h, r.w, 4), dtype=np.float32)
        stats = PtStats()
        self._check(self._lib.pt_render(self._ctx, C.byref(r), out.ctypes.data, 0, C.byref(stats) if want_stats else None))
        return out, stats

    def render_device(self, out_ptr, rect=None, want_stats=False):
        """Render into device memory (e.g. a torch CUDA tensor's data_ptr()); asynchronous unless want_stats."""
        r = PtRect(*rect) if rect is not None else None
        stats = PtStats()
        self._check(self._lib.pt_render(self._ctx, C.byref(r) if r is not None else None, C.c_void_p(out_ptr), 1, C.byref(stats) if want_stats else None))
        return stats

    def render_tiles(self, out_ptr, want_stats=False):
        stats = PtStats()
        self._check(self._lib.pt_render_tiles(self._ctx, C.c_void_p(out_ptr), C.byref(stats) if want_stats else None))
        return stats

    def unpack_tiles(self, gathered_ptr, max_tiles_per_rank, frame_ptr):
        self._check(self._lib.pt_unpack_tiles(self._ctx, C.c_void_p(gathered_ptr), max_tiles_per_rank, C.c_void_p(frame_ptr)))

    def unpack_tiles_ex(self, packed_ptr, part_stride_px, n_parts, first0, run, stride, frame_ptr):
        self._check(self._lib.pt_unpack_tiles_ex(self._ctx, C.c_void_p(packed_ptr), part_stride_px, n_parts, first0, run, stride, C.c_void_p(frame_ptr)))

    def set_textures(self, texture_set):
        """textures.TextureSet -> pt_set_textures (None removes all textures); call after set_scene"""
        if texture_set is None:
            self._check(self._lib.pt_set_textures(self._ctx, None, 0, None, None))
            return
        tex, n_tex, obj, rot = texture_set.as_ctypes()
        self._check(self._lib.pt_set_textures(self._ctx, C.cast(tex, C.c_void_p), n_tex, C.cast(obj, C.c_void_p), rot.ctypes.data))

    def update_rotations(self, rotations_xyzw):
        q = np.ascontiguousarray(rotations_xyzw, dtype=np.float32).reshape(-1, 4)
        self._check(self._lib.pt_update_rotations(self._ctx, q.ctypes.data, len(q)))

    def tonemap(self, hdr_ptr, n_pixels, params, out_ptr):
        """display transform (row N3): device float4[n] -> device packed uint32[n], asynchronous on the context's stream"""
        self._check(self._lib.pt_tonemap(self._ctx, C.c_void_p(hdr_ptr), n_pixels, C.addressof(params), C.c_void_p(out_ptr)))

    def accumulate(self, accum_ptr, radiance_ptr, n_pixels, frames_accumulated):
        """running mean of successive frames (device pointers), asynchronous on the context's stream"""
        self._check(self._lib.pt_accumulate(self._ctx, C.c_void_p(accum_ptr), C.c_void_p(radiance_ptr), n_pixels, frames_accumulated))

    def bloom(self, hdr_ptr, out_ptr, width, height, strength):
        """bloom (row N5): device float4[height * width] -> device float4[height * width] (out_ptr may equal hdr_ptr),
        asynchronous on the context's stream"""
        self._check(self._lib.pt_bloom(self._ctx, C.c_void_p(hdr_ptr), C.c_void_p(out_ptr), width, height, strength))

    def render_gbuffer_device(self, buffers, rect=None, previous_spheres=None, previous_rotations=None, previous=None):
        """G-buffer (row N6) of the frame the next render call renders.  buffers: {channel name: device pointer} (names of
        GBUFFER_CHANNELS; the others are not requested).  Asynchronous, ordered like the frame the next render call renders (with frames
        in flight: rotate over one set of buffers per lane); what is queued on the context's stream later sees the result.  previous_spheres (SPHERE_DTYPE[n]) / previous_rotations (float32[n, 4]): the previous
        pose the motion vectors are measured from, None = the current one.  previous="published": the pose published before the newest
        one (physics_publish), taken on the device (pt_render_gbuffer_published)."""
        if previous not in (None, "published"):
            raise ValueError(f"previous must be None or 'published', not {previous!r}")
        if previous == "published" and (previous_spheres is not None or previous_rotations is not None):
            raise ValueError("previous='published' takes no host pose")
        unknown = set(buffers) - {name for name, _ in GBUFFER_CHANNELS}
        if unknown:
            raise ValueError(f"unknown G-buffer channels {sorted(unknown)}")
        gb = PtGBuffer(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        r = PtRect(*rect) if rect is not None else None
        if previous == "published":
            self._check(self._lib.pt_render_gbuffer_published(self._ctx, C.byref(r) if r is not None else None, C.byref(gb)))
            return
        ps = np.ascontiguousarray(previous_spheres) if previous_spheres is not None else None
        pr = np.ascontiguousarray(previous_rotations, dtype=np.float32) if previous_rotations is not None else None
        self._check(self._lib.pt_render_gbuffer(self._ctx, C.byref(r) if r is not None else None, C.byref(gb),
                                                ps.ctypes.data if ps is not None else None, pr.ctypes.data if pr is not None else None))

    def render_gbuffer(self, channels="all", rect=None, previous_spheres=None, previous_rotations=None, fill=float("nan"), device=None, previous=None):
        """render_gbuffer_device into torch buffers filled with `fill` (what a pixel the pass does not write keeps) -> {channel:
        numpy float32 (h, w, width)} for the requested channels ("all" or names).  Synchronous."""
        import torch
        names = [name for name, _ in GBUFFER_CHANNELS] if channels == "all" else list(channels)
        width = dict(GBUFFER_CHANNELS)
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        w, h = rect[2], rect[3]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        bufs = {name: torch.full((h, w, width[name]), fill, dtype=torch.float32, device=dev) for name in names}
        torch.cuda.synchronize(dev)  # (filled on torch's stream, which the context's stream knows nothing of)
        self.render_gbuffer_device({name: b.data_ptr() for name, b in bufs.items()}, rect, previous_spheres, previous_rotations, previous)
        self.synchronize()
        return {name: b.cpu().numpy() for name, b in bufs.items()}

    def render_denoiser_device(self, mode, out_ptr, buffers, rect=None, want_stats=False):
        """A frame with the denoiser outputs of `mode` (row N7; abi_types.DENOISER_*) into device memory.  buffers: {output name: device
        pointer} (DENOISER_OUTPUTS[mode]; others are ignored, a missing one is the library's PT_ERR_INVALID_ARG).  Asynchronous unless
        want_stats; with frames in flight rotate over one set of buffers per lane, as for out."""
        r = PtRect(*rect) if rect is not None else None
        o = PtDenoiserOutputs(Denoiser=mode, **{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        stats = PtStats()
        self._check(self._lib.pt_render_denoiser(self._ctx, C.byref(r) if r is not None else None, C.c_void_p(out_ptr), 1, C.byref(o),
                                                 C.byref(stats) if want_stats else None))
        return stats

    def render_denoiser(self, mode, rect=None, fill=float("nan"), device=None):
        """render_denoiser_device into torch buffers filled with `fill` (what a pixel the frame does not write keeps) -> (out (h, w, 4),
        {output name: numpy float32 (h, w, width)}).  Synchronous."""
        import torch
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        w, h = rect[2], rect[3]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        # (filled from numpy: the fill's bits reach the buffers exactly, a NaN payload included)
        out = torch.from_numpy(np.full((h, w, 4), fill, dtype=np.float32)).to(dev)
        bufs = {name: torch.from_numpy(np.full((h, w, width), fill, dtype=np.float32)).to(dev) for name, width in DENOISER_OUTPUTS.get(mode, ())}
        torch.cuda.synchronize(dev)  # (filled on torch's stream, which the context's stream knows nothing of)
        self.render_denoiser_device(mode, out.data_ptr(), {name: b.data_ptr() for name, b in bufs.items()}, rect)
        self.synchronize()
        return out.cpu().numpy(), {name: b.cpu().numpy() for name, b in bufs.items()}

    def render_with_di_device(self, out_ptr, diffuse_ptr, specular_ptr, rect=None, mode=0, buffers=None, want_stats=False):
        """A frame whose direct illumination is supplied (pt_render_with_di): DI = Diffuse.rgb + Specular.rgb of the device float4 buffers (one per
        pixel of the rect) in place of row N4's estimate.  mode 0 = Denoiser::None (pt_render); else abi_types.DENOISER_* with `buffers` as
        for render_denoiser_device.  Asynchronous unless want_stats."""
        r = PtRect(*rect) if rect is not None else None
        di = PtDirectLighting(Diffuse=C.c_void_p(int(diffuse_ptr)), Specular=C.c_void_p(int(specular_ptr)))
        o = PtDenoiserOutputs(Denoiser=mode, **{name: C.c_void_p(int(ptr)) for name, ptr in (buffers or {}).items() if ptr}) if mode else None
        stats = PtStats()
        self._check(self._lib.pt_render_with_di(self._ctx, C.byref(r) if r is not None else None, C.c_void_p(out_ptr), 1, C.byref(di),
                                                C.byref(o) if o is not None else None, C.byref(stats) if want_stats else None))
        return stats

    def render_with_di(self, diffuse, specular, rect=None, mode=0, fill=float("nan"), device=None, alias=False):
        """render_with_di_device with the DI given as numpy float32 (h, w, 4) arrays (or torch CUDA tensors), into torch buffers filled with
        `fill` -> out (h, w, 4) numpy, or (out, {output name: numpy}) for a denoiser mode.  alias (NRD modes): the DI is placed in the
        frame's own Diffuse / Specular outputs, as the reference uses them.  Synchronous."""
        import torch
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        w, h = rect[2], rect[3]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)

        def on_device(a):
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
            return t.to(dev).reshape(h, w, 4).contiguous().clone()
        dd, ds = on_device(diffuse), on_device(specular)
        out = torch.from_numpy(np.full((h, w, 4), fill, dtype=np.float32)).to(dev)
        bufs = {name: torch.from_numpy(np.full((h, w, width), fill, dtype=np.float32)).to(dev) for name, width in DENOISER_OUTPUTS.get(mode, ())}
        if alias and mode in (2, 3):
            bufs = {"Diffuse": dd, "Specular": ds}
        torch.cuda.synchronize(dev)  # (filled on torch's stream, which the context's stream knows nothing of)
        self.render_with_di_device(out.data_ptr(), dd.data_ptr(), ds.data_ptr(), rect, mode, {name: b.data_ptr() for name, b in bufs.items()})
        self.synchronize()
        if not mode:
            return out.cpu().numpy()
        return out.cpu().numpy(), {name: b.cpu().numpy() for name, b in bufs.items()}

    def nrd_composition_device(self, mode, pack, width, height, buffers, hit_distance=NRD_REBLUR_HIT_DISTANCE):
        """NRD composition (row N8; mode abi_types.DENOISER_NRD_*): pack (before NRD, in place on NoisyDiffuse / NoisySpecular) or
        compose (after NRD, into Radiance) over width x height pixels.  buffers: {NRD_TEXTURES name: device pointer}; the ones the
        direction does not use may be left out.  hit_distance: ReBLUR's hit distance parameters.  Asynchronous on the context's stream."""
        unknown = set(buffers) - set(NRD_TEXTURES)
        if unknown:
            raise ValueError(f"unknown NRD composition buffers {sorted(unknown)}")
        k = PtNrdCompositionConstants(RenderSize=(C.c_uint32 * 2)(width, height), Pack=1 if pack else 0, Denoiser=mode,
                                      ReBLURHitDistance=(C.c_float * 4)(*hit_distance))
        t = PtNrdCompositionTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        self._check(self._lib.pt_nrd_composition(self._ctx, C.byref(k), C.byref(t)))

    def nrd_chain(self, mode, rect=None, denoise=None, hit_distance=NRD_REBLUR_HIT_DISTANCE, device=None):
        """The reference's NRD path for one frame (App.cpp:1140-1146, 1549-1642) with a stand-in for NRD: pt_render_gbuffer ->
        pt_render_denoiser (its buffers cleared to 0, as the reference's host clears them) -> pack -> denoise -> compose.  denoise(diffuse,
        specular) takes the packed torch buffers (h, w, 4) and returns the denoised pair; None = an identity copy.  Synchronous -> {name:
        numpy float32 (h, w, channels)}: the G-buffer inputs, Emission (pt_render_denoiser's out), NoisyDiffuse / NoisySpecular (as
        rendered), PackedDiffuse / PackedSpecular, DenoisedDiffuse / DenoisedSpecular and Radiance (the composed frame)."""
        import torch
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        w, h = rect[2], rect[3]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        width = dict(GBUFFER_CHANNELS)
        gb = {name: torch.zeros((h, w, width[name]), dtype=torch.float32, device=dev) for name in NRD_TEXTURES[:4]}
        guides = getattr(denoise, "gbuffer", {})  # G-buffer channels the denoiser reads besides these (NrdDenoiser: MotionVector)
        rad, nd, ns = (torch.zeros((h, w, 4), dtype=torch.float32, device=dev) for _ in range(3))
        torch.cuda.synchronize(dev)  # (cleared on torch's stream, which the context's stream knows nothing of)
        self.render_gbuffer_device(dict({name: b.data_ptr() for name, b in gb.items()}, **{name: b.data_ptr() for name, b in guides.items()}), rect,
                                   *getattr(denoise, "previous_pose", ()))
        self.render_denoiser_device(mode, rad.data_ptr(), {"Diffuse": nd.data_ptr(), "Specular": ns.data_ptr()}, rect)
        self.synchronize()
        res = {name: b.cpu().numpy() for name, b in gb.items()}
        res.update(Emission=rad.cpu().numpy(), NoisyDiffuse=nd.cpu().numpy(), NoisySpecular=ns.cpu().numpy())
        inputs = {name: b.data_ptr() for name, b in gb.items()}
        self.nrd_composition_device(mode, True, w, h, dict(inputs, NoisyDiffuse=nd.data_ptr(), NoisySpecular=ns.data_ptr()), hit_distance)
        self.synchronize()
        res.update(PackedDiffuse=nd.cpu().numpy(), PackedSpecular=ns.cpu().numpy())
        if hasattr(denoise, "gbuffer"):
            denoise.guides = gb
            res.update({name: b.cpu().numpy() for name, b in guides.items()})
        dd, ds = denoise(nd, ns) if denoise is not None else (nd.clone(), ns.clone())
        dd, ds = dd.contiguous(), ds.contiguous()
        torch.cuda.synchronize(dev)
        self.nrd_composition_device(mode, False, w, h, dict(inputs, DenoisedDiffuse=dd.data_ptr(), DenoisedSpecular=ds.data_ptr(), Radiance=rad.data_ptr()),
                                    hit_distance)
        self.synchronize()
        res.update(DenoisedDiffuse=dd.cpu().numpy(), DenoisedSpecular=ds.cpu().numpy(), Radiance=rad.cpu().numpy())
        return res

    def nrd_denoise_device(self, mode, width, height, buffers, accumulation_mode=0, frame_index=0, max_diffuse_frames=0, max_specular_frames=0,
                           atrous_iterations=0):
        """The NRD stand-in (row N9, DESIGN.md spec S15; mode abi_types.DENOISER_NRD_*) over width x height pixels: the packed In buffers
        -> the Out buffers compose reads, with the history the context keeps.  buffers: {NRD_DENOISE_TEXTURES name: device pointer}
        (BaseColorMetalness may be left out).  accumulation_mode: abi_types.NRD_ACCUMULATION_*.  Asynchronous on the context's stream."""
        unknown = set(buffers) - set(NRD_DENOISE_TEXTURES)
        if unknown:
            raise ValueError(f"unknown NRD denoise buffers {sorted(unknown)}")
        s = PtNrdDenoiseSettings(RenderSize=(C.c_uint32 * 2)(width, height), Denoiser=mode, AccumulationMode=accumulation_mode, FrameIndex=frame_index,
                                 MaxDiffuseFrames=max_diffuse_frames, MaxSpecularFrames=max_specular_frames, AtrousIterations=atrous_iterations)
        t = PtNrdDenoiseTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        self._check(self._lib.pt_nrd_denoise(self._ctx, C.byref(s), C.byref(t)))

    def nrd_reblur_device(self, width, height, buffers, **settings):
        """The ReBLUR stand-in (row N30, DESIGN.md spec S32) over width x height pixels: the In buffers pt_nrd_composition packed with
        DENOISER_NRD_REBLUR -> the Out buffers its compose reads, with a history of its own in the context (apart from nrd_denoise_device's).
        buffers: {NRD_DENOISE_TEXTURES name: device pointer} (BaseColorMetalness may be left out).  settings: abi_types.nrd_reblur_settings'
        keywords.  Asynchronous on the context's stream."""
        unknown = set(buffers) - set(NRD_DENOISE_TEXTURES)
        if unknown:
            raise ValueError(f"unknown NRD denoise buffers {sorted(unknown)}")
        s = nrd_reblur_settings(width, height, **settings)
        t = PtNrdDenoiseTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        self._check(self._lib.pt_nrd_reblur(self._ctx, C.byref(s), C.byref(t)))

    def nrd_reblur_history(self, width, height):
        """pt_nrd_reblur_history -> dict slow_d, slow_s, fast_d, fast_s, guide: the slot the last nrd_reblur_device call wrote, (h, w, 4) each"""
        out = {k: np.zeros((height, width, 4), np.float32) for k in ("slow_d", "slow_s", "fast_d", "fast_s", "guide")}
        self._check(self._lib.pt_nrd_reblur_history(self._ctx, *[a.ctypes.data for a in out.values()]))
        return out

    def restir_di_device(self, width, height, buffers, frame_index=0, reset_history=False, initial_samples=0, temporal=True, temporal_bias=1,
                         max_history=0, spatial=True, spatial_bias=1, spatial_samples=0, spatial_radius=0.0, light_sampling=None,
                         candidates=None, shading=None):
        """The reservoir pass that makes the DI render_with_di_device takes (row N10, DESIGN.md spec S16) over width x height pixels, for
        the frame the next render call renders: buffers = {RESTIR_DI_TEXTURES name: device pointer}, the G-buffer channels of
        render_gbuffer_device and the Diffuse / Specular outputs (float4; the caller clears them: pixels without DI are not written).
        *_bias: abi_types.RESTIR_BIAS_*; 0 for a count or the radius = the library's default.  The context keeps the history between
        calls.  Asynchronous, ordered like render_gbuffer_device; what is queued on the context's stream later sees the outputs.
        light_sampling: None = pt_restir_di (uniform candidates); a PtLightSamplingSettings or a dict of light_sampling_settings'
        arguments (mode = abi_types.LIGHT_SAMPLING_*, tile_size, tile_count, grid_size, lights_per_cell, build_samples, cell_size) =
        pt_restir_di_sampled (row N16, DESIGN.md spec S22).
        candidates: None = neither; a PtRestirDiCandidates or a dict of restir_di_candidates' arguments (brdf_samples, boiling_filter =
        the filter's strength) = pt_restir_di_ex (row N17, DESIGN.md spec S23).
        shading: not None = pt_restir_di_full (row N22, DESIGN.md spec S26), which also accepts RESTIR_BIAS_PAIRWISE: a PtRestirDiShading or
        a dict of restir_di_shading's arguments (reuse, max_age, max_distance; {} = reuse off)."""
        unknown = set(buffers) - set(RESTIR_DI_TEXTURES)
        if unknown:
            raise ValueError(f"unknown ReSTIR DI buffers {sorted(unknown)}")
        s = PtRestirDiSettings(RenderSize=(C.c_uint32 * 2)(width, height), FrameIndex=frame_index, ResetHistory=1 if reset_history else 0,
                               InitialSamples=initial_samples, EnableTemporal=int(temporal), TemporalBiasCorrection=temporal_bias,
                               MaxHistoryLength=max_history, EnableSpatial=int(spatial), SpatialBiasCorrection=spatial_bias,
                               SpatialSamples=spatial_samples, SpatialRadius=spatial_radius)
        t = PtRestirDiTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        ls = None
        if light_sampling is not None:
            ls = light_sampling if isinstance(light_sampling, PtLightSamplingSettings) else light_sampling_settings(**light_sampling)
        cd = None
        if candidates is not None:
            cd = candidates if isinstance(candidates, PtRestirDiCandidates) else restir_di_candidates(**candidates)
        if shading is not None:
            sh = shading if isinstance(shading, PtRestirDiShading) else restir_di_shading(**shading)
            self._check(self._lib.pt_restir_di_full(self._ctx, C.byref(s), C.byref(ls) if ls is not None else None, C.byref(cd) if cd is not None else None, C.byref(sh),
                                                    C.byref(t)))
        elif cd is not None:
            self._check(self._lib.pt_restir_di_ex(self._ctx, C.byref(s), C.byref(ls) if ls is not None else None, C.byref(cd), C.byref(t)))
        elif ls is None:
            self._check(self._lib.pt_restir_di(self._ctx, C.byref(s), C.byref(t)))
        else:
            self._check(self._lib.pt_restir_di_sampled(self._ctx, C.byref(s), C.byref(ls), C.byref(t)))

    def restir_di_history(self, width, height, which=0):
        """A slot of the reservoir pass's history (pt_restir_di_history; synchronous): which = 0 the slot the last restir_di_device call
        wrote, 1 the one before -> (planes (6, height * width, 4) float32: the surface record's four, the reservoir's two; transmission
        (height * width,)).  Pixels without a surface hold only plane 3."""
        planes, tr = np.zeros((6, height * width, 4), np.float32), np.zeros(height * width, np.float32)
        self._check(self._lib.pt_restir_di_history(self._ctx, which, planes.ctypes.data, tr.ctypes.data))
        return planes, tr

    def light_ris_download(self):
        """What the last restir_di_device call with a presampling mode built (pt_light_ris_download; synchronous) -> (pyramid float32
        (every level, leaves first), entries LIGHT_RIS_ENTRY_DTYPE (the Power_RIS segment, then the ReGIR segment))"""
        n_pyr, n_ris = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.pt_light_ris_download(self._ctx, None, C.byref(n_pyr), None, C.byref(n_ris)))
        pyramid, ris = np.zeros(n_pyr.value, np.float32), np.zeros(n_ris.value, LIGHT_RIS_ENTRY_DTYPE)
        self._check(self._lib.pt_light_ris_download(self._ctx, pyramid.ctypes.data, C.byref(n_pyr), ris.ctypes.data, C.byref(n_ris)))
        return pyramid, ris

    def restir_di(self, fill=float("nan"), device=None, previous_spheres=None, previous_rotations=None, **settings):
        """render_gbuffer_device + restir_di_device for the whole RenderSize into torch buffers (the outputs filled with `fill`, which
        pixels without DI keep) -> (diffuse, specular, gbuffer): two torch float32 (h, w, 4) tensors and {channel: tensor}.
        FrameIndex defaults to the constants'.  Synchronous."""
        import torch
        w, h = self._gs.RenderSize[0], self._gs.RenderSize[1]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        width = dict(GBUFFER_CHANNELS)
        gb = {name: torch.zeros((h, w, width[name]), dtype=torch.float32, device=dev) for name in RESTIR_DI_TEXTURES[:8]}
        dd, ds = (torch.from_numpy(np.full((h, w, 4), fill, dtype=np.float32)).to(dev) for _ in range(2))
        torch.cuda.synchronize(dev)  # (filled on torch's stream, which the context's stream knows nothing of)
        self.render_gbuffer_device({name: b.data_ptr() for name, b in gb.items()}, None, previous_spheres, previous_rotations)
        settings.setdefault("frame_index", self._gs.FrameIndex)
        self.restir_di_device(w, h, dict({name: b.data_ptr() for name, b in gb.items()}, Diffuse=dd.data_ptr(), Specular=ds.data_ptr()), **settings)
        self.synchronize()
        return dd, ds, gb

    def restir_di_full(self, shading=None, **kw):
        """restir_di through pt_restir_di_full (row N22): shading as restir_di_device takes it (None = reuse off); temporal_bias /
        spatial_bias may be RESTIR_BIAS_PAIRWISE"""
        return self.restir_di(shading={} if shading is None else shading, **kw)

    def render_sharc_device(self, out_ptr, rect=None, want_stats=False, **settings):
        """The frame through the radiance cache (row N14, DESIGN.md spec S20; pt_render_sharc) into device memory: settings = the fields of
        PtSharcSettings in snake case (capacity, downscale_factor, scene_scale, roughness_threshold, accumulation_frames, max_stale_frames,
        anti_firefly, visualize, reset_history, stages = SHARC_UPDATE | SHARC_RESOLVE | SHARC_QUERY); 0 = the library's default.  Runs on
        the lane of the next render call; asynchronous unless want_stats."""
        r = PtRect(*rect) if rect is not None else None
        s = sharc_settings(**settings)
        stats = PtStats()
        self._check(self._lib.pt_render_sharc(self._ctx, C.byref(r) if r is not None else None, C.c_void_p(out_ptr or 0), 1, C.byref(s),
                                              C.byref(stats) if want_stats else None))
        return stats

    def render_sharc(self, rect=None, want_stats=True, **settings):
        """render_sharc_device to a host numpy array (h, w, 4) float32 -> (image, stats); a call without the query stage returns
        (None, stats).  Synchronous."""
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        r = PtRect(*rect)
        s = sharc_settings(**settings)
        query = s.Stages == 0 or bool(s.Stages & 4)
        out = np.empty((r.h, r.w, 4), dtype=np.float32) if query else None
        stats = PtStats()
        self._check(self._lib.pt_render_sharc(self._ctx, C.byref(r), out.ctypes.data if query else None, 0, C.byref(s), C.byref(stats) if want_stats else None))
        if not want_stats:
            self.synchronize()
        return out, stats

    def render_lens_device(self, out_ptr, rect=None, want_stats=False):
        """The pure path-traced frame through the thin-lens camera (row N26, DESIGN.md spec S29; pt_render_lens) into device memory: the
        aperture is the camera's ApertureRadius (set_camera), the plane in focus lies at view depth |ForwardDirection|; aperture 0 is
        render_device's frame bit for bit.  Runs on the lane of the next render call; asynchronous unless want_stats."""
        r = PtRect(*rect) if rect is not None else None
        stats = PtStats()
        self._check(self._lib.pt_render_lens(self._ctx, C.byref(r) if r is not None else None, C.c_void_p(out_ptr or 0), 1, C.byref(stats) if want_stats else None))
        return stats

    def render_lens(self, rect=None, want_stats=True):
        """render_lens_device to a host numpy array (h, w, 4) float32 -> (image, stats).  Synchronous."""
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        r = PtRect(*rect)
        out = np.empty((r.h, r.w, 4), dtype=np.float32)
        stats = PtStats()
        self._check(self._lib.pt_render_lens(self._ctx, C.byref(r), out.ctypes.data, 0, C.byref(stats) if want_stats else None))
        if not want_stats:
            self.synchronize()
        return out, stats

    def render_gbuffer_packed_device(self, buffers, rect=None, previous_spheres=None, previous_rotations=None):
        """render_gbuffer_device into the reference's texel formats (row N27, DESIGN.md spec S30; pt_render_gbuffer_packed): buffers =
        {channel name: device pointer}, each rect.w * rect.h texels of abi_types.GBUFFER_PACKED, aligned to its texel.  Asynchronous, ordered
        like render_gbuffer_device."""
        unknown = set(buffers) - {name for name, _ in GBUFFER_CHANNELS}
        if unknown:
            raise ValueError(f"unknown G-buffer channels {sorted(unknown)}")
        gb = PtGBufferPacked(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        r = PtRect(*rect) if rect is not None else None
        ps = np.ascontiguousarray(previous_spheres) if previous_spheres is not None else None
        pr = np.ascontiguousarray(previous_rotations, dtype=np.float32) if previous_rotations is not None else None
        self._check(self._lib.pt_render_gbuffer_packed(self._ctx, C.byref(r) if r is not None else None, C.byref(gb),
                                                       ps.ctypes.data if ps is not None else None, pr.ctypes.data if pr is not None else None))

    def render_gbuffer_packed(self, channels="all", rect=None, previous_spheres=None, previous_rotations=None, fill=0xAB, device=None):
        """render_gbuffer_packed_device into torch buffers whose every byte is `fill` (what a texel the pass does not write keeps) ->
        {channel: numpy array (h, w, words) of the texel's raw words (abi_types.GBUFFER_PACKED)}.  Synchronous."""
        import torch
        names = [name for name, _ in GBUFFER_CHANNELS] if channels == "all" else list(channels)
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        w, h = rect[2], rect[3]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        shapes = {name: (GBUFFER_PACKED_DTYPE[name][0], GBUFFER_PACKED_DTYPE[name][1]) for name in names}
        bufs = {name: torch.full((h * w * width * np.dtype(dtype).itemsize,), fill, dtype=torch.uint8, device=dev) for name, (dtype, width) in shapes.items()}
        torch.cuda.synchronize(dev)  # (filled on torch's stream, which the context's stream knows nothing of)
        self.render_gbuffer_packed_device({name: b.data_ptr() for name, b in bufs.items()}, rect, previous_spheres, previous_rotations)
        self.synchronize()
        return {name: b.cpu().numpy().view(shapes[name][0]).reshape(h, w, shapes[name][1]) for name, b in bufs.items()}

    def render_from_gbuffer_device(self, out_ptr, inputs, fmt=0, rect=None, diffuse_ptr=None, specular_ptr=None, want_stats=False):
        """The pure path-traced frame whose first vertex is the G-buffer's texel instead of a traced ray (row N27, DESIGN.md spec S30;
        pt_render_from_gbuffer) into device memory.  inputs = {name: device pointer} for the eight channels of abi_types.GBUFFER_FRAME_INPUTS,
        rect-sized, in the float32 layouts of render_gbuffer_device (fmt 0) or the packed ones of render_gbuffer_packed_device (fmt 1);
        diffuse_ptr / specular_ptr: the DI as for render_with_di_device (None: no DI).  Runs on the lane of the next render call, after a
        G-buffer call queued there just before without a wait; asynchronous unless want_stats."""
        r = PtRect(*rect) if rect is not None else None
        unknown = set(inputs) - set(GBUFFER_FRAME_INPUTS)
        if unknown:
            raise ValueError(f"unknown G-buffer frame inputs {sorted(unknown)}")
        gi = PtGBufferInput(Format=fmt, **{name: C.c_void_p(int(ptr)) for name, ptr in inputs.items() if ptr})
        di = PtDirectLighting(Diffuse=C.c_void_p(int(diffuse_ptr or 0)), Specular=C.c_void_p(int(specular_ptr or 0))) if diffuse_ptr or specular_ptr else None
        stats = PtStats()
        self._check(self._lib.pt_render_from_gbuffer(self._ctx, C.byref(r) if r is not None else None, C.c_void_p(out_ptr or 0), 1, C.byref(gi),
                                                     C.byref(di) if di is not None else None, C.byref(stats) if want_stats else None))
        return stats

    def render_from_gbuffer(self, inputs, fmt=0, rect=None, di=None, device=None):
        """render_from_gbuffer_device with the inputs given as numpy arrays {name: array} (float32 for fmt 0, the raw words render_gbuffer_packed
        returns for fmt 1) and di = None or (diffuse, specular) float32 (h, w, 4) -> (image (h, w, 4) float32, stats).  Synchronous."""
        import torch
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        w, h = rect[2], rect[3]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)

        def on_device(a):
            return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev)
        bufs = {name: on_device(a) for name, a in inputs.items()}
        dd, ds = (on_device(np.asarray(a, dtype=np.float32)) for a in di) if di is not None else (None, None)
        out = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)  # (filled on torch's stream, which the context's stream knows nothing of)
        stats = self.render_from_gbuffer_device(out.data_ptr(), {name: b.data_ptr() for name, b in bufs.items()}, fmt, rect,
                                                dd.data_ptr() if dd is not None else None, ds.data_ptr() if ds is not None else None, want_stats=True)
        return out.cpu().numpy(), stats

    def render_sharc_ex_device(self, out_ptr, diffuse_ptr=None, specular_ptr=None, rect=None, mode=0, buffers=None, want_stats=False, **settings):
        """render_sharc_device with the frame's direct illumination and denoiser outputs (row N18, DESIGN.md spec S24; pt_render_sharc_ex).
        diffuse_ptr / specular_ptr: the DI as for render_with_di_device (None: no DI); mode 0 = Denoiser::None, else abi_types.DENOISER_*
        with `buffers` as for render_denoiser_device.  Without DI and mode the call is render_sharc_device.  anti_firefly=True (row N19,
        spec S25) is accepted here, with or without DI and mode; render_sharc_device refuses it.  Asynchronous unless want_stats."""
        r = PtRect(*rect) if rect is not None else None
        s = sharc_settings(**settings)
        di = PtDirectLighting(Diffuse=C.c_void_p(int(diffuse_ptr or 0)), Specular=C.c_void_p(int(specular_ptr or 0))) if diffuse_ptr or specular_ptr else None
        o = PtDenoiserOutputs(Denoiser=mode, **{name: C.c_void_p(int(ptr)) for name, ptr in (buffers or {}).items() if ptr}) if mode else None
        stats = PtStats()
        self._check(self._lib.pt_render_sharc_ex(self._ctx, C.byref(r) if r is not None else None, C.c_void_p(out_ptr or 0), 1, C.byref(s),
                                                 C.byref(di) if di is not None else None, C.byref(o) if o is not None else None,
                                                 C.byref(stats) if want_stats else None))
        return stats

    def render_sharc_ex(self, diffuse=None, specular=None, rect=None, mode=0, fill=float("nan"), device=None, alias=False, **settings):
        """render_sharc_ex_device with the DI given as numpy float32 (h, w, 4) arrays or torch CUDA tensors (None: no DI), into torch
        buffers filled with `fill` -> (out (h, w, 4) numpy or None without the query stage, {output name: numpy}, stats).  alias (NRD
        modes): the DI is placed in the frame's own Diffuse / Specular outputs, as the reference uses them.  Synchronous."""
        import torch
        if rect is None:
            rect = (0, 0, self._gs.RenderSize[0], self._gs.RenderSize[1])
        w, h = rect[2], rect[3]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)

        def on_device(a):
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
            return t.to(dev).reshape(h, w, 4).contiguous().clone()
        dd, ds = (on_device(diffuse), on_device(specular)) if diffuse is not None else (None, None)
        out = torch.from_numpy(np.full((h, w, 4), fill, dtype=np.float32)).to(dev)
        bufs = {name: torch.from_numpy(np.full((h, w, width), fill, dtype=np.float32)).to(dev) for name, width in DENOISER_OUTPUTS.get(mode, ())}
        if alias and mode in (2, 3) and dd is not None:
            bufs = {"Diffuse": dd, "Specular": ds}
        torch.cuda.synchronize(dev)  # (filled on torch's stream, which the context's stream knows nothing of)
        stats = self.render_sharc_ex_device(out.data_ptr(), dd.data_ptr() if dd is not None else None, ds.data_ptr() if ds is not None else None, rect, mode,
                                            {name: b.data_ptr() for name, b in bufs.items()}, want_stats=True, **settings)
        self.synchronize()
        s = sharc_settings(**settings)
        query = s.Stages == 0 or bool(s.Stages & 4)
        return (out.cpu().numpy() if query else None), {name: b.cpu().numpy() for name, b in bufs.items()}, stats

    def sharc_download(self, capacity):
        """The cache as the last render_sharc call left it (pt_sharc_download) -> (keys uint64[capacity], voxels uint32[capacity, 4])"""
        keys, voxels = np.zeros(capacity, np.uint64), np.zeros((capacity, 4), np.uint32)
        self._check(self._lib.pt_sharc_download(self._ctx, keys.ctypes.data, voxels.ctypes.data, capacity))
        return keys, voxels

    def sharc_upload(self, keys, voxels):
        """Installs a cache made elsewhere (pt_sharc_upload): keys uint64[capacity], voxels uint32[capacity, 4]"""
        keys, voxels = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(voxels, np.uint32)
        assert voxels.shape == (len(keys), 4)
        self._check(self._lib.pt_sharc_upload(self._ctx, keys.ctypes.data, voxels.ctypes.data, len(keys)))

    def upscale_device(self, input_size, output_size, buffers, jitter=(0.0, 0.0), reset=False, max_history_weight=0.0):
        """The super-resolution stand-in (row N11, DESIGN.md spec S17): Color / Depth / Velocity at input_size = (w, h) -> Output at
        output_size = (W, H), with the history the context keeps.  buffers: {UPSCALE_TEXTURES name: device pointer}.  jitter: what the
        reference hands XeSS, -PtCamera.Jitter.  Asynchronous on the context's stream."""
        unknown = set(buffers) - set(UPSCALE_TEXTURES)
        if unknown:
            raise ValueError(f"unknown upscale buffers {sorted(unknown)}")
        s = PtUpscaleSettings(InputSize=(C.c_uint32 * 2)(*input_size), OutputSize=(C.c_uint32 * 2)(*output_size), Jitter=(C.c_float * 2)(*jitter),
                              Reset=1 if reset else 0, MaxHistoryWeight=max_history_weight)
        t = PtUpscaleTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        self._check(self._lib.pt_upscale(self._ctx, C.byref(s), C.byref(t)))

    def nis_sharpen_device(self, size, buffers, sharpness=0.5, hdr_mode=0):
        """The sharpening stand-in (row N12, DESIGN.md spec S18): Color -> Output, both float4 at size = (w, h), the output size.
        buffers: {NIS_TEXTURES name: device pointer}; Output must not overlap Color.  sharpness in [0, 1] (the reference's default 0.5);
        hdr_mode: abi_types.NIS_HDR_NONE (what the reference passes) or NIS_HDR_LINEAR.  Asynchronous on the context's stream."""
        unknown = set(buffers) - set(NIS_TEXTURES)
        if unknown:
            raise ValueError(f"unknown NIS buffers {sorted(unknown)}")
        s = PtNisSettings(Size=(C.c_uint32 * 2)(*size), Sharpness=sharpness, HdrMode=hdr_mode)
        t = PtNisTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        self._check(self._lib.pt_nis_sharpen(self._ctx, C.byref(s), C.byref(t)))

    def chromatic_aberration_device(self, size, buffers, focus_uv=CHROMATIC_ABERRATION_FOCUS_UV, offsets=CHROMATIC_ABERRATION_OFFSETS):
        """Chromatic aberration (row N29, DESIGN.md spec S31): Color -> Output, both float4 at size = (w, h); between nis_sharpen_device and
        bloom in the post chain.  buffers: {CHROMATIC_ABERRATION_TEXTURES name: device pointer}; Output must not overlap Color.  focus_uv
        in [0, 1]^2; offsets: the factor of r, g, b, each within +-1/16 (channel c is magnified by 1 + offsets[c] about the focus).
        Asynchronous on the context's stream."""
        unknown = set(buffers) - set(CHROMATIC_ABERRATION_TEXTURES)
        if unknown:
            raise ValueError(f"unknown chromatic aberration buffers {sorted(unknown)}")
        s = PtChromaticAberrationSettings(Size=(C.c_uint32 * 2)(*size), FocusUV=(C.c_float * 2)(*focus_uv), Offsets=(C.c_float * 3)(*offsets))
        t = PtChromaticAberrationTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        self._check(self._lib.pt_chromatic_aberration(self._ctx, C.byref(s), C.byref(t)))

    def frame_gen_device(self, render_size, output_size, buffers, fmt=0, reset=False):
        """The frame-interpolation stand-in (row N13, DESIGN.md spec S19): the frame half way between the previous call's frame and this
        one.  buffers: {FRAME_GEN_TEXTURES name: device pointer}: Color and Output packed uint32 at output_size = (W, H) (pt_tonemap's
        out), Depth (float) and MotionVector (float3) at render_size = (w, h); Output must not overlap an input.  fmt:
        abi_types.FRAME_GEN_RGBA8 or FRAME_GEN_RGB10A2.  Returns True when a frame was generated, False on a restart (the first call,
        reset, a change of a size or of fmt), where Output is Color.  Asynchronous on the context's stream."""
        unknown = set(buffers) - set(FRAME_GEN_TEXTURES)
        if unknown:
            raise ValueError(f"unknown frame generation buffers {sorted(unknown)}")
        s = PtFrameGenSettings(RenderSize=(C.c_uint32 * 2)(*render_size), OutputSize=(C.c_uint32 * 2)(*output_size), Format=fmt, Reset=1 if reset else 0)
        t = PtFrameGenTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        generated = C.c_uint32(0)
        self._check(self._lib.pt_frame_gen(self._ctx, C.byref(s), C.byref(t), C.byref(generated)))
        return bool(generated.value)

    def ray_reconstruction_device(self, render_size, output_size, buffers, camera, jitter=None, reset=False, max_history_weight=0.0):
        """The ray-reconstruction stand-in (row N15, DESIGN.md spec S21): the noisy radiance of render_denoiser's mode 1 with the
        G-buffer's guides at render_size = (w, h) -> the denoised Output at output_size = (W, H), with the history the context keeps.
        buffers: {RAY_RECONSTRUCTION_TEXTURES name: device pointer}; Output must not overlap an input.  camera: the frame's PtCamera
        (host.camera_matrices), whose Position and matrices travel by value; jitter: -PtCamera.Jitter unless given.  Asynchronous on
        the context's stream."""
        unknown = set(buffers) - set(RAY_RECONSTRUCTION_TEXTURES)
        if unknown:
            raise ValueError(f"unknown ray reconstruction buffers {sorted(unknown)}")
        s = ray_reconstruction_settings(render_size, output_size, camera, jitter, reset, max_history_weight)
        t = PtRayReconstructionTextures(**{name: C.c_void_p(int(ptr)) for name, ptr in buffers.items() if ptr})
        self._check(self._lib.pt_ray_reconstruction(self._ctx, C.byref(s), C.byref(t)))

    def ray_reconstruction_history(self, output_size):
        """The history slot the last ray_reconstruction_device call wrote (pt_ray_reconstruction_history; synchronous) ->
        (history (H, W, 4), normal (H, W, 4), depth (H, W)) float32"""
        W, H = output_size
        hist, nrm, z = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
        self._check(self._lib.pt_ray_reconstruction_history(self._ctx, hist.ctypes.data, nrm.ctypes.data, z.ctypes.data))
        return hist, nrm, z

    def upscaler(self, output_size, mode=0, device=None, **settings):
        """An `upscale(color, depth, velocity, jitter)` that keeps the sizes and settings across frames and runs pt_upscale (row N11):
        output_size = (W, H); mode: abi_types.UPSCALE_* (its `input_size` is the RenderSize to render at).  settings: upscale_device's
        keywords.  Successive frames continue the context's history; `reset()` makes the next frame restart it."""
        return Upscaler(self, output_size, mode, device, settings)

    def nrd_denoiser(self, mode, rect=None, device=None, **settings):
        """A `denoise(diffuse, specular)` for nrd_chain that runs pt_nrd_denoise (row N9) in place of the identity copy: it carries the
        MotionVector buffer nrd_chain fills (its `gbuffer` attribute) and the G-buffer's LinearDepth / NormalRoughness it is handed
        there.  Successive frames of one denoiser continue the context's history; `restart()` makes the next frame CLEAR_AND_RESTART.
        settings: nrd_denoise_device's keywords.  `previous_pose` = (previous_spheres, previous_rotations) for the next G-buffer."""
        return NrdDenoiser(self, mode, rect, device, settings)

    def nrd_reblur_denoiser(self, rect=None, device=None, **settings):
        """nrd_denoiser's counterpart backed by pt_nrd_reblur (row N30): a `denoise(diffuse, specular)` for nrd_chain(DENOISER_NRD_REBLUR).
        settings: nrd_reblur_device's keywords; `frame_index` advances by one per call from the value given (default 0)."""
        return NrdDenoiser(self, 2, rect, device, settings, reblur=True)

    def pack_rgb(self, src_ptr, n_pixels, dst_ptr):
        """device float4[n] -> device 3 floats per pixel (the 12-byte exchange format)"""
        self._check(self._lib.pt_pack_rgb(self._ctx, C.c_void_p(src_ptr), n_pixels, C.c_void_p(dst_ptr)))

    def unpack_tiles_rgb(self, packed_ptr, part_stride_px, n_parts, first0, run, stride, frame_ptr):
        self._check(self._lib.pt_unpack_tiles_rgb(self._ctx, C.c_void_p(packed_ptr), part_stride_px, n_parts, first0, run, stride, C.c_void_p(frame_ptr)))

    def trace_rays(self, origins, directions, tmin=0.0, use_bvh=True):
        """pt_trace_rays -> (t, ids): closest hits against the scene the next render call renders (after update_spheres: the moved spheres and
        the refitted tree of that frame's lane); use_bvh=False runs the brute-force kernel.  Does not count as a frame."""
        o =np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        t = np.empty(n, dtype=np.float32)
        ids = np.empty(n, dtype=np.uint32)
        self._check(self._lib.pt_trace_rays(self._ctx, o.ctypes.data, d.ctypes.data, n, tmin, 1 if use_bvh else 0, t.ctypes.data, ids.ctypes.data))
        return t, ids

    def trace_rays_stats(self, origins, directions, tmin=0.0):
        """-> (t, ids, visits) with visits[:, 0] = internal nodes visited, visits[:, 1] = spheres tested per ray; the scene is trace_rays'"""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        t = np.empty(n, dtype=np.float32)
        ids = np.empty(n, dtype=np.uint32)
        visits = np.zeros((n, 2), dtype=np.uint32)
        self._check(self._lib.pt_trace_rays_stats(self._ctx, o.ctypes.data, d.ctypes.data, n, tmin, t.ctypes.data, ids.ctypes.data, visits.ctypes.data))
        return t, ids, visits

    def download_accel(self):
        """-> (nodes, order): the binary tree the next render call walks (after update_spheres: the refitted tree of that frame's lane) and its
        leaf order"""
        n = self.accel.node_count
        nodes = np.zeros(n, dtype=BVH_NODE_DTYPE)
        self._check(self._lib.pt_accel_download(self._ctx, nodes.ctypes.data, n))
        order = np.zeros(self.accel.leaf_count, dtype=np.uint32)
        self._check(self._lib.pt_accel_download_order(self._ctx, order.ctypes.data, len(order)))
        return nodes, order

    def download_wide(self):
        """The 4-wide view of the tree (pt_accel_download_wide) -> (node_count, 16) uint32, record i in row i (rows of odd-depth
        nodes are zero); None when the scene is not walked through one (LDS-resident, a single node, PT_WIDE=0)."""
        n = self.accel.node_count
        words = np.zeros((max(n, 1), 16), dtype=np.uint32)
        has = C.c_uint32(0)
        self._check(self._lib.pt_accel_download_wide(self._ctx, words.ctypes.data, n, C.byref(has)))
        return words[:n] if has.value else None


def sharc_settings(capacity=0, downscale_factor=0, scene_scale=0.0, roughness_threshold=0.0, accumulation_frames=0, max_stale_frames=0, anti_firefly=False,
                   visualize=False, reset_history=False, stages=0):
    """PtSharcSettings from keywords (0 = the library's default)"""
    return PtSharcSettings(Capacity=capacity, DownscaleFactor=downscale_factor, SceneScale=scene_scale, RoughnessThreshold=roughness_threshold,
                           AccumulationFrames=accumulation_frames, MaxStaleFrames=max_stale_frames, IsAntiFireflyEnabled=1 if anti_firefly else 0,
                           IsHashGridVisualizationEnabled=1 if visualize else 0, ResetHistory=1 if reset_history else 0, Stages=stages)


class NrdDenoiser:
    """Renderer.nrd_denoiser / nrd_reblur_denoiser: the `denoise` callable nrd_chain takes, backed by pt_nrd_denoise or (reblur) pt_nrd_reblur."""

    def __init__(self, renderer, mode, rect, device, settings, reblur=False):
        import torch
        self._r, self.mode, self.settings, self.reblur = renderer, mode, dict(settings), reblur
        self.frame_index = self.settings.pop("frame_index", 0) if reblur else 0
        if rect is None:
            rect = (0, 0, renderer._gs.RenderSize[0], renderer._gs.RenderSize[1])
        self.w, self.h = rect[2], rect[3]
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.gbuffer = {"MotionVector": torch.zeros((self.h, self.w, 3), dtype=torch.float32, device=dev)}
        self.guides = None
        self.previous_pose = ()
        self._restart = True

    def restart(self):
        self._restart = True

    def __call__(self, diffuse, specular):
        import torch
        od, os_ = torch.empty_like(diffuse), torch.empty_like(specular)
        od.copy_(diffuse)  # (misses are never written: they keep the packed value, as the identity chain does)
        os_.copy_(specular)
        torch.cuda.synchronize(diffuse.device)
        mode = 2 if self._restart else self.settings.get("accumulation_mode", 0)
        settings = dict(self.settings, accumulation_mode=mode)
        buffers = dict(ViewZ=self.guides["LinearDepth"].data_ptr(), MotionVector=self.gbuffer["MotionVector"].data_ptr(),
                       NormalRoughness=self.guides["NormalRoughness"].data_ptr(), InDiffuse=diffuse.data_ptr(), InSpecular=specular.data_ptr(),
                       OutDiffuse=od.data_ptr(), OutSpecular=os_.data_ptr())
        if self.reblur:
            self._r.nrd_reblur_device(self.w, self.h, buffers, frame_index=self.frame_index, **settings)
            self.frame_index += 1
        else:
            self._r.nrd_denoise_device(self.mode, self.w, self.h, buffers, **settings)
        self._r.synchronize()
        self._restart = False
        return od, os_


class Upscaler:
    """Renderer.upscaler: render at `input_size`, then call with the frame's torch buffers -> the torch float32 (H, W, 4) frame at
    output size, backed by pt_upscale."""

    def __init__(self, renderer, output_size, mode, device, settings):
        import torch
        self._r, self.mode, self.settings = renderer, mode, dict(settings)
        self.output_size = tuple(int(x) for x in output_size)
        self.input_size = load_hip().upscale_input_size(mode, *self.output_size)
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.output = torch.zeros((self.output_size[1], self.output_size[0], 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self._reset = True

    def reset(self):
        self._reset = True

    def __call__(self, color, depth, velocity, jitter=(0.0, 0.0)):
        """color (h, w, 4), depth (h, w[, 1]), velocity (h, w, 3): contiguous torch float32 CUDA tensors the context's stream may read
        (synchronise torch's stream first if it wrote them).  jitter: -PtCamera.Jitter.  Asynchronous; returns `output`."""
        self._r.upscale_device(self.input_size, self.output_size, dict(Color=color.data_ptr(), Depth=depth.data_ptr(), Velocity=velocity.data_ptr(),
                                                                       Output=self.output.data_ptr()),
                               jitter=jitter, reset=self._reset or self.settings.get("reset", False),
                               **{k: v for k, v in self.settings.items() if k != "reset"})
        self._reset = False
        return self.output
