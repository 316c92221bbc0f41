// RTXDI.hpp -- C++ host mirror of the reference's RTXDI pass object as App::Impl::Render drives it (Source/App.cpp:1187-1227:
// RTXDI::SetConstants, then RTXDI::Render between the G-buffer pass and the frame) over pt_restir_di (row N10, DESIGN.md spec S16), a
// stand-in for the RTXDI SDK, which the reference does not vendor.  The settings are the subset of ReSTIRDI_Parameters
// (Source/MyAppData.h:190-250) the stand-in reads; resources are DEVICE pointers of RenderSize texels (the layouts of
// PtRestirDiTextures) instead of D3D12 textures.  With a local-light sampling mode other than Uniform the passes run through
// pt_restir_di_sampled (row N16, spec S22: Power_RIS tiles and the ReGIR grid, MyAppData.h:194-218); with BRDF candidates or the boiling
// filter through pt_restir_di_ex (row N17, spec S23: MyAppData.h:220-221, 229-235).  After the SetConstants overload that takes
// ShadingSettings the passes run through pt_restir_di_full (row N22, spec S26), which accepts Pairwise and reuses final visibility.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>

#include "Raytracing.hpp"

namespace dxrs {

enum class ReSTIRDI_BiasCorrectionMode : uint32_t { Off = 0, Basic = 1, Pairwise = 2, Raytraced = 3 };

enum class ReSTIRDI_LocalLightSamplingMode : uint32_t { Uniform = 0, Power_RIS = 1, ReGIR_RIS = 2 };

struct ReSTIRDISettings {  // MyAppData.h:190-250 (IsEnabled = true is the reference's default frame)
    struct {  // MyAppData.h:194-208: Cell.Size in [0.1, 10], BuildSamples at most 32 (the cell visualisation is not built)
        struct { float Size = 1; } Cell;
        uint32_t BuildSamples = 8;
    } ReGIR;
    // LocalLightMode: the reference's default is ReGIR_RIS (MyAppData.h:212); this mirror's stays Uniform, so that a host written
    // against row N10 keeps the frames it had
    // BRDFSamples (at most 8) and BoilingFilter: the reference's defaults are 1 and {true, 0.2} (MyAppData.h:220-221, 229-235); this
    // mirror's stay off for the same reason -- ReferenceDefaults() below is the reference's whole block
    struct { ReSTIRDI_LocalLightSamplingMode LocalLightMode = ReSTIRDI_LocalLightSamplingMode::Uniform; uint32_t LocalLightSamples = 8; uint32_t BRDFSamples = 0; } InitialSampling;
    struct {
        bool IsEnabled = true; ReSTIRDI_BiasCorrectionMode BiasCorrectionMode = ReSTIRDI_BiasCorrectionMode::Basic; uint32_t MaxHistoryLength = 20;
        struct { bool IsEnabled = false; float Strength = 0.2f; } BoilingFilter;
    } TemporalResampling;
    struct { bool IsEnabled = true; ReSTIRDI_BiasCorrectionMode BiasCorrectionMode = ReSTIRDI_BiasCorrectionMode::Basic; uint32_t Samples = 1; float Radius = 32; } SpatialResampling;

    // the reference's default ReSTIRDI block: ReGIR_RIS candidates, 8 local + 1 BRDF candidate, the boiling filter at strength 0.2
    static ReSTIRDISettings ReferenceDefaults()
    {
        ReSTIRDISettings s;
        s.InitialSampling.LocalLightMode = ReSTIRDI_LocalLightSamplingMode::ReGIR_RIS;
        s.InitialSampling.BRDFSamples = 1;
        s.TemporalResampling.BoilingFilter.IsEnabled = true;
        s.TemporalResampling.BoilingFilter.Strength = 0.2f;
        return s;
    }
};

// ReSTIRDI_ShadingParameters' final-visibility reuse, which the reference leaves at the SDK's defaults (Source/RTXDI.ixx:134; on, 4
// frames and 16 pixels as recollected); this mirror's reuse stays off so that a host keeps the frames it had
struct ShadingSettings {
    bool ReuseFinalVisibility = false;
    uint32_t MaxAge = 4;
    float MaxDistance = 16;
};

class RTXDI {
public:
    // the G-buffer textures RAB_GetGBufferSurface reads and the two textures DIFinalShading writes
    struct Textures {
        const void *Position{}, *GeometricNormal{}, *LinearDepth{}, *MotionVector{}, *BaseColorMetalness{}, *NormalRoughness{}, *IOR{}, *Transmission{};
        void *Diffuse{}, *Specular{};
    } GPUBuffers;

    explicit RTXDI(DeviceContext& deviceContext) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    // RTXDI::SetConstants(settings, resetHistory, renderSize, frameIndex)
    void SetConstants(const ReSTIRDISettings& settings, bool resetHistory, std::array<uint32_t, 2> renderSize, uint32_t frameIndex)
    {
        m_settings = PtRestirDiSettings{};
        m_settings.RenderSize[0] = renderSize[0];
        m_settings.RenderSize[1] = renderSize[1];
        m_settings.FrameIndex = frameIndex;
        m_settings.ResetHistory = resetHistory ? 1u : 0u;
        m_settings.InitialSamples = settings.InitialSampling.LocalLightSamples;
        m_settings.EnableTemporal = settings.TemporalResampling.IsEnabled ? 1u : 0u;
        m_settings.TemporalBiasCorrection = static_cast<uint32_t>(settings.TemporalResampling.BiasCorrectionMode);
        m_settings.MaxHistoryLength = settings.TemporalResampling.MaxHistoryLength;
        m_settings.EnableSpatial = settings.SpatialResampling.IsEnabled ? 1u : 0u;
        m_settings.SpatialBiasCorrection = static_cast<uint32_t>(settings.SpatialResampling.BiasCorrectionMode);
        m_settings.SpatialSamples = settings.SpatialResampling.Samples;
        m_settings.SpatialRadius = settings.SpatialResampling.Radius;
        m_sampling = PtLightSamplingSettings{};  // (tile and grid sizes: the library's defaults)
        m_sampling.Mode = static_cast<uint32_t>(settings.InitialSampling.LocalLightMode);
        m_sampling.ReGIRBuildSamples = settings.ReGIR.BuildSamples;
        m_sampling.ReGIRCellSize = settings.ReGIR.Cell.Size;
        m_candidates = PtRestirDiCandidates{};
        m_candidates.BrdfSamples = settings.InitialSampling.BRDFSamples;
        m_candidates.EnableBoilingFilter = settings.TemporalResampling.BoilingFilter.IsEnabled ? 1u : 0u;
        m_candidates.BoilingFilterStrength = settings.TemporalResampling.BoilingFilter.Strength;
        m_full = false;
    }

    // ... with the shading parameters: Render() then goes through pt_restir_di_full, where BiasCorrectionMode may be Pairwise
    void SetConstants(const ReSTIRDISettings& settings, const ShadingSettings& shading, bool resetHistory, std::array<uint32_t, 2> renderSize, uint32_t frameIndex)
    {
        SetConstants(settings, resetHistory, renderSize, frameIndex);
        m_shading = PtRestirDiShading{};
        m_shading.ReuseFinalVisibility = shading.ReuseFinalVisibility ? 1u : 0u;
        m_shading.FinalVisibilityMaxAge = shading.MaxAge;
        m_shading.FinalVisibilityMaxDistance = shading.MaxDistance;
        m_full = true;
    }

    // RTXDI::Render: the DI passes of the frame the next render call renders, asynchronous
    void Render()
    {
        const PtRestirDiTextures t{ GPUBuffers.Position, GPUBuffers.GeometricNormal, GPUBuffers.LinearDepth, GPUBuffers.MotionVector,
                                    GPUBuffers.BaseColorMetalness, GPUBuffers.NormalRoughness, GPUBuffers.IOR, GPUBuffers.Transmission,
                                    GPUBuffers.Diffuse, GPUBuffers.Specular };
        if (m_full) ThrowIfFailed(pt_restir_di_full(m_ctx, &m_settings, &m_sampling, &m_candidates, &m_shading, &t), m_ctx, "pt_restir_di_full");
        else if (m_candidates.BrdfSamples || m_candidates.EnableBoilingFilter)
            ThrowIfFailed(pt_restir_di_ex(m_ctx, &m_settings, &m_sampling, &m_candidates, &t), m_ctx, "pt_restir_di_ex");
        else if (m_sampling.Mode == PT_LIGHT_SAMPLING_UNIFORM) ThrowIfFailed(pt_restir_di(m_ctx, &m_settings, &t), m_ctx, "pt_restir_di");
        else ThrowIfFailed(pt_restir_di_sampled(m_ctx, &m_settings, &m_sampling, &t), m_ctx, "pt_restir_di_sampled");
    }

private:
    PtContext* m_ctx;
    PtRestirDiSettings m_settings{};
    PtLightSamplingSettings m_sampling{};
    PtRestirDiCandidates m_candidates{};
    PtRestirDiShading m_shading{};
    bool m_full = false;
};

}  // namespace dxrs
