// Raytracing.hpp -- host mirror of the reference's pass objects for this path, on top of the C-ABI:
//   Raytracing        Source/Raytracing.ixx:29-112  { GraphicsSettings, SetConstants(...) noexcept, Render(...) }
//                     Render(..., SHARC&, SHARCSettings) Source/Raytracing.ixx:114-148 (SHARC.hpp; row N14)
//   (GBufferGeneration Source/GBufferGeneration.ixx:27-117 is folded in: Render traces the primary hit too.)
// Same names, argument meaning and error behaviour: errors surface as C++ exceptions
// (reference: ThrowIfFailed -> std::system_error, Source/ErrorHelpers.ixx:16-32); SetConstants is noexcept.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pt_api.h"
#include "Camera.hpp"
#include "HaltonSampler.hpp"
#include "SHARC.hpp"
#include "Scene.hpp"

namespace dxrs {

enum class Denoiser : uint32_t { None, DLSSRayReconstruction, NRDReBLUR, NRDReLAX };  // Source/Denoiser.ixx

inline void ThrowIfFailed(PtStatus status, PtContext* ctx, const char* what)
{
    if (status != PT_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(static_cast<int>(status)) + "): " + pt_last_error(ctx));
}

// Stand-in for the reference's DeviceContext/CommandList pair: owns the PtContext (device, stream, device memory).
class DeviceContext {
public:
    explicit DeviceContext(int device = 0, uint32_t flags = 0, uint64_t stream = 0, uint32_t tileSize = 0)
    {
        PtConfig config{};
        config.device = device; config.flags = flags; config.stream = stream; config.tile_size = tileSize;
        PtContext* ctx = nullptr;
        const PtStatus st = pt_create(&config, &ctx);
        if (st != PT_OK) throw std::runtime_error("pt_create failed (" + std::to_string(static_cast<int>(st)) + "): no usable HIP device");
        m_ctx.reset(ctx);
    }
    PtContext* Get() const noexcept { return m_ctx.get(); }

private:
    struct Deleter { void operator()(PtContext* p) const noexcept { pt_destroy(p); } };
    std::unique_ptr<PtContext, Deleter> m_ctx;
};

struct Raytracing {
    struct GraphicsSettings {  // Raytracing.ixx:30-36
        UInt2 RenderSize;
        uint32_t FrameIndex{}, Bounces{}, SamplesPerPixel{};
        float ThroughputThreshold = 1e-3f;
        bool IsRussianRouletteEnabled{}, IsShaderExecutionReorderingEnabled{}, IsDIEnabled{};
        dxrs::Denoiser Denoiser = dxrs::Denoiser::None;
    };

    struct SHARCSettings : SHARC::Constants {  // Raytracing.ixx:38-42; the values of MyAppData.h:256-265
        uint32_t DownscaleFactor = 4;
        float RoughnessThreshold = 0.4f;
        uint32_t IsHashGridVisualizationEnabled{};
    };

    explicit Raytracing(DeviceContext& deviceContext) noexcept(false) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    // Scene::Load/Refresh + CreateAccelerationStructures (Scene.ixx:123-284)
    PtAccelInfo SetScene(const Scene& scene)
    {
        const auto sd = scene.GetSceneData();
        ThrowIfFailed(pt_set_scene(m_ctx, scene.GetSpheres().data(), scene.GetMaterials().data(), scene.GetObjectCount(), &sd), m_ctx, "pt_set_scene");
        PtAccelInfo info{};
        ThrowIfFailed(pt_build_accel(m_ctx, &info), m_ctx, "pt_build_accel");
        if (scene.HasTextures()) {  // ObjectData::TextureMapInfoArray + the texture uploads of Scene::Load (Scene.ixx:150-180)
            std::vector<PtTexture> textures;
            for (const auto& t : scene.GetTextures()) textures.push_back(t.ToPt());
            ThrowIfFailed(pt_set_textures(m_ctx, textures.data(), static_cast<uint32_t>(textures.size()), scene.GetObjectTextures().data(),
                                          scene.GetRotations().data()), m_ctx, "pt_set_textures");
        }
        return info;
    }

    // the poses of a running scene (MyScene::Tick -> Scene::Refresh): rotations only orient texture coordinates
    void UpdateRotations(const Scene& scene)
    {
        if (scene.HasTextures())
            ThrowIfFailed(pt_update_rotations(m_ctx, scene.GetRotations().data(), scene.GetObjectCount()), m_ctx, "pt_update_rotations");
    }

    void SetCamera(const Camera& camera)
    {
        const auto cam = ToPt(camera);
        ThrowIfFailed(pt_set_camera(m_ctx, &cam), m_ctx, "pt_set_camera");
    }

    void SetConstants(const GraphicsSettings& graphicsSettings) noexcept  // Raytracing.ixx:92-104
    {
        m_graphicsSettings = PtGraphicsSettings{};
        m_graphicsSettings.RenderSize[0] = graphicsSettings.RenderSize.x;
        m_graphicsSettings.RenderSize[1] = graphicsSettings.RenderSize.y;
        m_graphicsSettings.FrameIndex = graphicsSettings.FrameIndex;
        m_graphicsSettings.Bounces = graphicsSettings.Bounces;
        m_graphicsSettings.SamplesPerPixel = graphicsSettings.SamplesPerPixel;
        m_graphicsSettings.ThroughputThreshold = graphicsSettings.ThroughputThreshold;
        m_graphicsSettings.IsRussianRouletteEnabled = graphicsSettings.IsRussianRouletteEnabled;
        m_graphicsSettings.IsShaderExecutionReorderingEnabled = graphicsSettings.IsShaderExecutionReorderingEnabled;
        m_graphicsSettings.IsDIEnabled = graphicsSettings.IsDIEnabled;
        m_graphicsSettings.Denoiser = static_cast<uint32_t>(graphicsSettings.Denoiser);
    }

    // the constants alone (what Render does first): for callers that dispatch through the tile entry points (TileExchange.hpp)
    void UploadConstants() { ThrowIfFailed(pt_set_constants(m_ctx, &m_graphicsSettings), m_ctx, "pt_set_constants"); }

    // Raytracing::Render (Raytracing.ixx:106-112): uploads the constants, then DispatchRays(W, H, 1).
    // radiance: W*H float4 host buffer (the reference's Radiance texture, kept at fp32).
    PtStats Render(std::vector<Float4>& radiance)
    {
        ThrowIfFailed(pt_set_constants(m_ctx, &m_graphicsSettings), m_ctx, "pt_set_constants");
        radiance.resize(static_cast<size_t>(m_graphicsSettings.RenderSize[0]) * m_graphicsSettings.RenderSize[1]);
        PtStats stats{};
        ThrowIfFailed(pt_render(m_ctx, nullptr, radiance.data(), 0, &stats), m_ctx, "pt_render");
        return stats;
    }

    // The outputs Raytracing.hlsl writes besides the radiance when GraphicsSettings.Denoiser != None (App.cpp:1140-1146, 1230-1263):
    // DEVICE buffers of W*H texels, cleared by the caller as the reference's host clears its textures.  DLSSRayReconstruction writes
    // SpecularHitDistance (float); NRDReBLUR / NRDReLAX write Diffuse and Specular (float4, 16-byte aligned).
    struct DenoiserBuffers {
        void* Diffuse = nullptr;
        void* Specular = nullptr;
        void* SpecularHitDistance = nullptr;
    };

    // Raytracing::Render of a frame for the denoiser GraphicsSettings.Denoiser names (row N7, pt_render_denoiser).  The library takes the
    // mode per frame, not in the constants: they go up with Denoiser = None.  Render(radiance) keeps refusing a denoiser, as
    // pt_set_constants does.
    PtStats Render(std::vector<Float4>& radiance, DenoiserBuffers& buffers)
    {
        if (m_graphicsSettings.Denoiser == 0) throw std::invalid_argument("Raytracing::Render: GraphicsSettings.Denoiser is None (use Render(radiance))");
        PtGraphicsSettings constants = m_graphicsSettings;
        constants.Denoiser = 0;
        ThrowIfFailed(pt_set_constants(m_ctx, &constants), m_ctx, "pt_set_constants");
        radiance.resize(static_cast<size_t>(m_graphicsSettings.RenderSize[0]) * m_graphicsSettings.RenderSize[1]);
        PtDenoiserOutputs outputs{};
        outputs.Denoiser = m_graphicsSettings.Denoiser;
        outputs.Diffuse = buffers.Diffuse;
        outputs.Specular = buffers.Specular;
        outputs.SpecularHitDistance = buffers.SpecularHitDistance;
        PtStats stats{};
        ThrowIfFailed(pt_render_denoiser(m_ctx, nullptr, radiance.data(), 0, &outputs, &stats), m_ctx, "pt_render_denoiser");
        return stats;
    }

    // The textures the ReSTIR-DI passes write for Raytracing.hlsl to read as DI (DIFinalShading.hlsl:95-104): DEVICE float4 buffers of
    // W*H texels, 16-byte aligned.  They may be the frame's own DenoiserBuffers, as the reference uses them.
    struct DirectLighting {
        const void* Diffuse = nullptr;
        const void* Specular = nullptr;
    };

    // Raytracing::Render with IsDIEnabled = isReSTIRDIEnabled (App.cpp:1262; pt_render_with_di): DI = Diffuse.rgb + Specular.rgb
    // in place of the library's own estimate.  buffers: the denoiser outputs when GraphicsSettings.Denoiser names one (required then).
    PtStats Render(std::vector<Float4>& radiance, const DirectLighting& di, DenoiserBuffers* buffers = nullptr)
    {
        PtGraphicsSettings constants = m_graphicsSettings;
        constants.Denoiser = 0;
        ThrowIfFailed(pt_set_constants(m_ctx, &constants), m_ctx, "pt_set_constants");
        radiance.resize(static_cast<size_t>(m_graphicsSettings.RenderSize[0]) * m_graphicsSettings.RenderSize[1]);
        PtDirectLighting lighting{};
        lighting.Diffuse = di.Diffuse;
        lighting.Specular = di.Specular;
        PtDenoiserOutputs outputs{};
        if (m_graphicsSettings.Denoiser != 0) {
            if (!buffers) throw std::invalid_argument("Raytracing::Render: GraphicsSettings.Denoiser needs its DenoiserBuffers");
            outputs.Denoiser = m_graphicsSettings.Denoiser;
            outputs.Diffuse = buffers->Diffuse;
            outputs.Specular = buffers->Specular;
            outputs.SpecularHitDistance = buffers->SpecularHitDistance;
        }
        PtStats stats{};
        ThrowIfFailed(pt_render_with_di(m_ctx, nullptr, radiance.data(), 0, &lighting, m_graphicsSettings.Denoiser != 0 ? &outputs : nullptr, &stats),
                      m_ctx, "pt_render_with_di");
        return stats;
    }

    // Raytracing::Render(commandList, tlas, SHARC&, SHARCSettings) (Raytracing.ixx:114-148; row N14, pt_render_sharc): the sparse update
    // pass, the resolve and the frame through the cache.  The context owns the cache the reference's SHARC object owns.
    // settings.IsAntiFireflyEnabled (App.cpp:1278 sets it; row N19, spec S25): pt_render_sharc refuses the filter, so such a frame goes
    // through pt_render_sharc_ex, without DI or denoiser outputs unless GraphicsSettings.Denoiser names one (which then needs the
    // five-argument form and its buffers).
    PtStats Render(std::vector<Float4>& radiance, SHARC& sharc, const SHARCSettings& settings)
    {
        if (settings.IsAntiFireflyEnabled) return Render(radiance, sharc, settings, nullptr, nullptr);
        ThrowIfFailed(pt_set_constants(m_ctx, &m_graphicsSettings), m_ctx, "pt_set_constants");
        radiance.resize(static_cast<size_t>(m_graphicsSettings.RenderSize[0]) * m_graphicsSettings.RenderSize[1]);
        PtSharcSettings s{};
        s.Capacity = sharc.GetCapacity();
        s.DownscaleFactor = settings.DownscaleFactor;
        s.SceneScale = settings.SceneScale;
        s.RoughnessThreshold = settings.RoughnessThreshold;
        s.AccumulationFrames = settings.AccumulationFrames;
        s.MaxStaleFrames = settings.MaxStaleFrames;
        s.IsAntiFireflyEnabled = settings.IsAntiFireflyEnabled ? 1u : 0u;
        s.IsHashGridVisualizationEnabled = settings.IsHashGridVisualizationEnabled;
        s.ResetHistory = sharc.NeedsReset() ? 1u : 0u;
        PtStats stats{};
        ThrowIfFailed(pt_render_sharc(m_ctx, nullptr, radiance.data(), 0, &s, &stats), m_ctx, "pt_render_sharc");
        sharc.ClearReset();  // (only now: a call that threw has restarted nothing)
        return stats;
    }

    // The same with IsDIEnabled = isReSTIRDIEnabled and GraphicsSettings.Denoiser (App.cpp:1255-1268; row N18, pt_render_sharc_ex): the
    // reference's default frame.  di: null = no DI; buffers: the denoiser outputs when GraphicsSettings.Denoiser names one (required
    // then).  The constants go up with Denoiser = None, the mode travels with the call.  settings.IsAntiFireflyEnabled reaches the
    // filter (row N19, spec S25) here.
    PtStats Render(std::vector<Float4>& radiance, SHARC& sharc, const SHARCSettings& settings, const DirectLighting* di, DenoiserBuffers* buffers)
    {
        PtGraphicsSettings constants = m_graphicsSettings;
        constants.Denoiser = 0;
        ThrowIfFailed(pt_set_constants(m_ctx, &constants), m_ctx, "pt_set_constants");
        radiance.resize(static_cast<size_t>(m_graphicsSettings.RenderSize[0]) * m_graphicsSettings.RenderSize[1]);
        PtSharcSettings s{};
        s.Capacity = sharc.GetCapacity();
        s.DownscaleFactor = settings.DownscaleFactor;
        s.SceneScale = settings.SceneScale;
        s.RoughnessThreshold = settings.RoughnessThreshold;
        s.AccumulationFrames = settings.AccumulationFrames;
        s.MaxStaleFrames = settings.MaxStaleFrames;
        s.IsAntiFireflyEnabled = settings.IsAntiFireflyEnabled ? 1u : 0u;
        s.IsHashGridVisualizationEnabled = settings.IsHashGridVisualizationEnabled;
        s.ResetHistory = sharc.NeedsReset() ? 1u : 0u;
        PtDirectLighting lighting{};
        if (di) {
            lighting.Diffuse = di->Diffuse;
            lighting.Specular = di->Specular;
        }
        PtDenoiserOutputs outputs{};
        if (m_graphicsSettings.Denoiser != 0) {
            if (!buffers) throw std::invalid_argument("Raytracing::Render: GraphicsSettings.Denoiser needs its DenoiserBuffers");
            outputs.Denoiser = m_graphicsSettings.Denoiser;
            outputs.Diffuse = buffers->Diffuse;
            outputs.Specular = buffers->Specular;
            outputs.SpecularHitDistance = buffers->SpecularHitDistance;
        }
        PtStats stats{};
        ThrowIfFailed(pt_render_sharc_ex(m_ctx, nullptr, radiance.data(), 0, &s, di ? &lighting : nullptr, m_graphicsSettings.Denoiser != 0 ? &outputs : nullptr, &stats),
                      m_ctx, "pt_render_sharc_ex");
        sharc.ClearReset();
        return stats;
    }

    // The pure path-traced frame through Camera::GenerateThinLensRay (Camera.hlsli:43-54, which the reference declares and never calls;
    // row N26, spec S29, pt_render_lens): the aperture is the ApertureRadius of the camera last given to pt_set_camera (the reference's
    // controller has no setter: callers write Camera::ApertureRadius), the plane in focus what CameraController::SetFocusDistance set.
    // ApertureRadius == 0 is Render(radiance), bit for bit.
    PtStats RenderThinLens(std::vector<Float4>& radiance)
    {
        ThrowIfFailed(pt_set_constants(m_ctx, &m_graphicsSettings), m_ctx, "pt_set_constants");
        radiance.resize(static_cast<size_t>(m_graphicsSettings.RenderSize[0]) * m_graphicsSettings.RenderSize[1]);
        PtStats stats{};
        ThrowIfFailed(pt_render_lens(m_ctx, nullptr, radiance.data(), 0, &stats), m_ctx, "pt_render_lens");
        return stats;
    }

    // The G-buffer textures Raytracing.hlsl:118-148 loads as the primary surface of every sample (App.cpp:1235-1268 binds them; row N27,
    // spec S30): DEVICE buffers of W*H texels in the float32 layouts of GBufferGeneration::Textures (Packed = false) or in the
    // reference's formats (GBufferGeneration::PackedTextures).
    struct GBufferTextures {
        bool Packed = false;
        const void *Position = nullptr, *FlatNormal = nullptr, *GeometricNormal = nullptr, *BaseColorMetalness = nullptr, *NormalRoughness = nullptr, *IOR = nullptr,
                   *Transmission = nullptr, *Radiance = nullptr;
    };

    // Raytracing::Render as the reference's raygen shader runs it, Denoiser::None: no primary ray, the first vertex of every sample is the
    // G-buffer's texel (pt_render_from_gbuffer).  di: IsDIEnabled with its two textures, nullptr = off.
    PtStats Render(std::vector<Float4>& radiance, const GBufferTextures& gbuffer, const DirectLighting* di = nullptr)
    {
        PtGraphicsSettings constants = m_graphicsSettings;
        constants.Denoiser = 0;
        constants.IsDIEnabled = di ? 1 : 0;
        ThrowIfFailed(pt_set_constants(m_ctx, &constants), m_ctx, "pt_set_constants");
        radiance.resize(static_cast<size_t>(m_graphicsSettings.RenderSize[0]) * m_graphicsSettings.RenderSize[1]);
        PtGBufferInput in{};
        in.Format = gbuffer.Packed ? 1u : 0u;
        in.Position = gbuffer.Position; in.FlatNormal = gbuffer.FlatNormal; in.GeometricNormal = gbuffer.GeometricNormal;
        in.BaseColorMetalness = gbuffer.BaseColorMetalness; in.NormalRoughness = gbuffer.NormalRoughness; in.IOR = gbuffer.IOR;
        in.Transmission = gbuffer.Transmission; in.Radiance = gbuffer.Radiance;
        PtDirectLighting lighting{};
        if (di) { lighting.Diffuse = di->Diffuse; lighting.Specular = di->Specular; }
        PtStats stats{};
        ThrowIfFailed(pt_render_from_gbuffer(m_ctx, nullptr, radiance.data(), 0, &in, di ? &lighting : nullptr, &stats), m_ctx, "pt_render_from_gbuffer");
        return stats;
    }

private:
    PtContext* m_ctx;
    PtGraphicsSettings m_graphicsSettings{};
};

}  // namespace dxrs
