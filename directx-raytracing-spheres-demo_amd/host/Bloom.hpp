// Bloom.hpp -- C++ host mirror of PostProcessing::Bloom (Source/Bloom.ixx) and its settings (Source/MyAppData.h:305-311, 368):
// the pass object the reference's App::Impl::ProcessBloom (Source/App.cpp:1723-1729) drives, over pt_bloom (row N5).
#pragma once

#include <algorithm>
#include <stdexcept>

#include "Raytracing.hpp"

namespace dxrs::PostProcessing {

struct Bloom {
    struct Constants { float Strength; };  // Bloom::Constants

    // GraphicsSettings.PostProcessing.Bloom: on by default, Strength 0.05, clamped to [0, 1] when the settings are loaded
    struct Settings {
        bool IsEnabled = true;
        float Strength = 0.05f;
        void Clamp() { Strength = std::clamp(Strength, 0.0f, 1.0f); }
    };

    explicit Bloom(DeviceContext& deviceContext) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    // SetTextures(input, output): width x height float4 DEVICE buffers (output may be input); the blur chain lives in the context
    void SetTextures(const void* input, void* output, UInt2 size)
    {
        m_input = input;
        m_output = output;
        m_size = size;
    }

    // Process: the chain and the merge, asynchronous on the context's stream
    void Process(Constants constants)
    {
        ThrowIfFailed(pt_bloom(m_ctx, m_input, m_output, m_size.x, m_size.y, constants.Strength), m_ctx, "pt_bloom");
    }

private:
    PtContext* m_ctx;
    const void* m_input = nullptr;
    void* m_output = nullptr;
    UInt2 m_size;
};

}  // namespace dxrs::PostProcessing
