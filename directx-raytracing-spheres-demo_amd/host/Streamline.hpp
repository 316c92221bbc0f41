// Streamline.hpp -- C++ host mirror of the NIS subset of the reference's Streamline wrapper (Source/Streamline.ixx: IsAvailable,
// SetConstants(NISOptions) -> slNISSetOptions, Tag, Evaluate) as App::ProcessNIS uses it (Source/App.cpp:1710-1721), over pt_nis_sharpen
// (row N12, DESIGN.md spec S18), a stand-in for Streamline's NIS plugin, which the reference does not vendor.  The names below are the
// subset of the SDK's API that ProcessNIS touches, on this file's own types; resources are DEVICE pointers (the layouts of
// PtNisTextures) instead of D3D12 textures, and the extent of the two tagged buffers is handed to Evaluate.
// Not built: the DLSS features of Streamline.ixx (DLSS, DLSS_G, DLSS_RR -- IsAvailable answers false for them and Evaluate refuses
// them), PCL / Reflex markers, frame tokens, sl::Constants, NIS's scaler mode and its PQ HDR mode.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>

#include "Raytracing.hpp"

namespace dxrs {

namespace sl {

enum class Feature : uint32_t { DLSS, DLSS_G, DLSS_RR, NIS, PCL, Reflex };
enum class Result : int32_t { eOk = 0, eErrorInvalidParameter = -1, eErrorFeatureNotSupported = -2, eErrorMissingInputParameter = -3 };
enum class NISMode : uint32_t { eOff, eScaler, eSharpen };
enum class NISHDR : uint32_t { eNone, eLinear, ePQ };  // the values are PtNisSettings.HdrMode
enum class BufferType : uint32_t { ScalingInputColor, ScalingOutputColor, Count };

struct NISOptions {
    NISMode mode = NISMode::eScaler;
    float sharpness = 0.0f;
    NISHDR hdrMode = NISHDR::eNone;
};

struct Extent { uint32_t width, height; };

}  // namespace sl

class Streamline {
public:
    explicit Streamline(DeviceContext& deviceContext) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    // NIS is the one feature of Streamline.ixx's list with a stand-in here; the DLSS features are not built
    bool IsAvailable(sl::Feature feature) const { return feature == sl::Feature::NIS; }

    sl::Result SetConstants(const sl::NISOptions& options)
    {
        m_NISOptions = options;
        return sl::Result::eOk;
    }

    void Tag(sl::BufferType type, const void* devicePointer) { m_resources[static_cast<size_t>(type)] = devicePointer; }

    // kFeatureNIS in sharpen mode: one pt_nis_sharpen call, asynchronous on the context's stream; `extent` = the size of both tags
    sl::Result Evaluate(sl::Feature feature, sl::Extent extent)
    {
        if (!IsAvailable(feature)) return sl::Result::eErrorFeatureNotSupported;
        if (m_NISOptions.mode == sl::NISMode::eOff) return sl::Result::eOk;
        if (m_NISOptions.mode != sl::NISMode::eSharpen) return sl::Result::eErrorFeatureNotSupported;  // the scaler is not built
        PtNisSettings s{};
        s.Size[0] = extent.width;
        s.Size[1] = extent.height;
        s.Sharpness = m_NISOptions.sharpness;
        s.HdrMode = static_cast<uint32_t>(m_NISOptions.hdrMode);
        const PtNisTextures t{ m_resources[static_cast<size_t>(sl::BufferType::ScalingInputColor)],
                               const_cast<void*>(m_resources[static_cast<size_t>(sl::BufferType::ScalingOutputColor)]) };
        if (!t.Color || !t.Output) return sl::Result::eErrorMissingInputParameter;  // a tag is missing: nothing is called
        const PtStatus st = pt_nis_sharpen(m_ctx, &s, &t);
        if (st == PT_ERR_INVALID_ARG) return sl::Result::eErrorInvalidParameter;
        if (st == PT_ERR_UNSUPPORTED) return sl::Result::eErrorFeatureNotSupported;
        ThrowIfFailed(st, m_ctx, "pt_nis_sharpen");
        return sl::Result::eOk;
    }

private:
    PtContext* m_ctx;
    std::array<const void*, static_cast<size_t>(sl::BufferType::Count)> m_resources{};
    sl::NISOptions m_NISOptions{};
};

}  // namespace dxrs
