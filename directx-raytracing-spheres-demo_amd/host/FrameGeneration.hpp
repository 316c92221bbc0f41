// FrameGeneration.hpp -- C++ host mirror of what the reference does for DLSS frame generation (App::SetFrameGenerationOptions ->
// slDLSSGSetOptions, App::ProcessDLSSFrameGeneration's three tags, Source/App.cpp:1673-1680) over pt_frame_gen (row N13, DESIGN.md spec
// S19), a stand-in for Streamline's DLSS-G plugin, which the reference does not vendor.  The plugin presents its frame by itself;
// here Generate writes it into a buffer of the caller's.  Resources are DEVICE pointers (the layouts of PtFrameGenTextures) instead of
// D3D12 textures.  host/Streamline.hpp keeps reporting DLSS_G as unavailable: this class is the stand-in's own interface.
// Not built: UI / HUD colour tags, pacing, Reflex markers, more than one generated frame (numFramesToGenerate is always 1).
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>

#include "Raytracing.hpp"

namespace dxrs {

namespace sl {
enum class DLSSGMode : uint32_t { eOff, eOn, eAuto };
}

class FrameGeneration {
public:
    enum class BufferType : uint32_t { Depth, MotionVectors, HUDLessColor, Count };
    enum class Format : uint32_t { R8G8B8A8_UNORM, R10G10B10A2_UNORM };  // the values are PtFrameGenSettings.Format
    enum class Result : int32_t { eOk = 0, eErrorInvalidParameter = -1, eErrorMissingInputParameter = -3 };
    struct Extent { uint32_t width, height; };

    explicit FrameGeneration(DeviceContext& deviceContext) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    // slDLSSGSetOptions: switching the feature on again restarts the history, as the reference's m_resetHistory does
    void SetOptions(sl::DLSSGMode mode)
    {
        if (mode != sl::DLSSGMode::eOff && m_mode == sl::DLSSGMode::eOff) m_reset = true;
        m_mode = mode;
    }

    void SetFormat(Format format) { m_format = format; }
    void ResetHistory() { m_reset = true; }
    void Tag(BufferType type, const void* devicePointer) { m_resources[static_cast<size_t>(type)] = devicePointer; }

    // One pt_frame_gen call, asynchronous on the context's stream: `output` receives the frame between the previous call's frame and
    // the tagged one.  generated = false where there is no such frame yet (eOff, the first call, a reset, a change of size or format):
    // `output` is then the tagged colour, or untouched with eOff.
    Result Generate(Extent renderExtent, Extent outputExtent, void* output, bool& generated)
    {
        generated = false;
        if (m_mode == sl::DLSSGMode::eOff) return Result::eOk;
        PtFrameGenSettings s{};
        s.RenderSize[0] = renderExtent.width; s.RenderSize[1] = renderExtent.height;
        s.OutputSize[0] = outputExtent.width; s.OutputSize[1] = outputExtent.height;
        s.Format = static_cast<uint32_t>(m_format);
        s.Reset = m_reset ? 1u : 0u;
        const PtFrameGenTextures t{ m_resources[static_cast<size_t>(BufferType::HUDLessColor)], m_resources[static_cast<size_t>(BufferType::Depth)],
                                    m_resources[static_cast<size_t>(BufferType::MotionVectors)], output };
        if (!t.Color || !t.Depth || !t.MotionVector || !t.Output) return Result::eErrorMissingInputParameter;  // a tag is missing: nothing is called
        uint32_t made = 0;
        const PtStatus st = pt_frame_gen(m_ctx, &s, &t, &made);
        if (st == PT_ERR_INVALID_ARG) return Result::eErrorInvalidParameter;
        ThrowIfFailed(st, m_ctx, "pt_frame_gen");
        m_reset = false;
        generated = made != 0;
        return Result::eOk;
    }

    Result Generate(Extent renderExtent, Extent outputExtent, void* output)
    {
        bool generated = false;
        return Generate(renderExtent, outputExtent, output, generated);
    }

private:
    PtContext* m_ctx;
    std::array<const void*, static_cast<size_t>(BufferType::Count)> m_resources{};
    sl::DLSSGMode m_mode = sl::DLSSGMode::eOff;
    Format m_format = Format::R8G8B8A8_UNORM;
    bool m_reset = true;
};

}  // namespace dxrs
