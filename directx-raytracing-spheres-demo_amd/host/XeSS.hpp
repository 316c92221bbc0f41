// XeSS.hpp -- C++ host mirror of the reference's XeSS wrapper (Source/XeSS.ixx: GetInputResolution, Tag, SetConstants, Execute) over
// pt_upscale (row N11, DESIGN.md spec S17), a stand-in for the XeSS SDK, which the reference does not vendor.  The xess_* names below
// are the subset of the SDK's API that App::SetSuperResolutionOptions and App::ProcessXeSSSuperResolution (Source/App.cpp:1434-1447,
// 1682-1708) use; resources are DEVICE pointers (the layouts of PtUpscaleTextures) instead of D3D12 textures.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>

#include "Raytracing.hpp"

namespace dxrs {

struct xess_2d_t { uint32_t x, y; };
// the SDK's quality settings App::SetSuperResolutionOptions selects from; the values are pt_upscale_input_size's modes
enum xess_quality_settings_t : uint32_t {
    XESS_QUALITY_SETTING_AA = 1, XESS_QUALITY_SETTING_QUALITY = 2, XESS_QUALITY_SETTING_BALANCED = 3, XESS_QUALITY_SETTING_PERFORMANCE = 4,
    XESS_QUALITY_SETTING_ULTRA_PERFORMANCE = 5
};
enum xess_result_t : int32_t { XESS_RESULT_SUCCESS = 0, XESS_RESULT_ERROR_INVALID_ARGUMENT = -1 };

enum class XeSSResourceType { Depth, Velocity, ExposureScale, ResponsivePixelMask, Color, Output };

struct XeSSSettings {
    xess_2d_t InputSize{};
    float Jitter[2]{};
    float ExposureScale = 1;  // accepted, not read by S17
    bool Reset{};
};

// SuperResolutionMode (Source/MyAppData.h) and the Auto rule of App::SetSuperResolutionOptions, through pt_upscale_input_size (mode 0)
enum class SuperResolutionMode : uint32_t { Auto, Native, Quality, Balanced, Performance, UltraPerformance };

class XeSS {
public:
    XeSS(DeviceContext& deviceContext, xess_2d_t outputResolution, uint32_t flags = 0) : m_ctx(deviceContext.Get()), m_outputResolution(outputResolution)
    {
        (void)flags;  // the SDK's init flags (depth and velocity conventions) have no counterpart: S17 fixes both
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    bool IsAvailable() const { return true; }

    xess_result_t GetInputResolution(xess_quality_settings_t quality, xess_2d_t& resolution) const
    {
        return pt_upscale_input_size(static_cast<uint32_t>(quality), m_outputResolution.x, m_outputResolution.y, &resolution.x, &resolution.y) == PT_OK
                   ? XESS_RESULT_SUCCESS : XESS_RESULT_ERROR_INVALID_ARGUMENT;
    }

    // SelectSuperResolutionMode + the switch of App::SetSuperResolutionOptions in one call
    xess_result_t GetInputResolution(SuperResolutionMode mode, xess_2d_t& resolution) const
    {
        return pt_upscale_input_size(static_cast<uint32_t>(mode), m_outputResolution.x, m_outputResolution.y, &resolution.x, &resolution.y) == PT_OK
                   ? XESS_RESULT_SUCCESS : XESS_RESULT_ERROR_INVALID_ARGUMENT;
    }

    void Tag(XeSSResourceType type, const void* devicePointer) { m_resources[static_cast<size_t>(type)] = devicePointer; }

    void SetConstants(const XeSSSettings& settings) { m_settings = settings; }

    // the history cap of the stand-in (not an SDK call): 0 = the library's default
    void SetMaxHistoryWeight(float weight) { m_maxHistoryWeight = weight; }

    // one pt_upscale call, asynchronous on the context's stream; ExposureScale and ResponsivePixelMask tags are accepted and ignored
    xess_result_t Execute()
    {
        PtUpscaleSettings s{};
        s.InputSize[0] = m_settings.InputSize.x;
        s.InputSize[1] = m_settings.InputSize.y;
        s.OutputSize[0] = m_outputResolution.x;
        s.OutputSize[1] = m_outputResolution.y;
        s.Jitter[0] = m_settings.Jitter[0];
        s.Jitter[1] = m_settings.Jitter[1];
        s.Reset = m_settings.Reset ? 1u : 0u;
        s.MaxHistoryWeight = m_maxHistoryWeight;
        auto r = [&](XeSSResourceType t) { return m_resources[static_cast<size_t>(t)]; };
        const PtUpscaleTextures t{ r(XeSSResourceType::Color), r(XeSSResourceType::Depth), r(XeSSResourceType::Velocity),
                                   const_cast<void*>(r(XeSSResourceType::Output)) };
        const PtStatus st = pt_upscale(m_ctx, &s, &t);
        if (st == PT_ERR_INVALID_ARG) return XESS_RESULT_ERROR_INVALID_ARGUMENT;
        ThrowIfFailed(st, m_ctx, "pt_upscale");
        return XESS_RESULT_SUCCESS;
    }

private:
    PtContext* m_ctx;
    xess_2d_t m_outputResolution;
    std::array<const void*, 6> m_resources{};
    XeSSSettings m_settings{};
    float m_maxHistoryWeight = 0.0f;
};

}  // namespace dxrs
