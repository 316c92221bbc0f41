// ChromaticAberration.hpp -- C++ host mirror of the reference's "Chromatic Aberration" post-processing setting (README.md:59, between
// NVIDIA Image Scaling and Bloom), in the pass-object pattern of Bloom.hpp, over pt_chromatic_aberration (row N29).  The reference tree
// at hand holds no source for the pass, so the names follow PostProcessing::Bloom and the arithmetic is DESIGN.md spec S31.
#pragma once

#include <algorithm>
#include <stdexcept>

#include "Raytracing.hpp"

namespace dxrs::PostProcessing {

struct ChromaticAberration {
    struct Constants {
        Float2 FocusUV{ 0.5f, 0.5f };
        // A recollection of the defaults of upstream's later revision, not read from the reference tree at hand.
        float Offsets[3] = { 0.003f, 0.003f, -0.003f };
    };

    // on by default with the constants above; the library accepts |offset| <= 1/16 and a focus inside the image
    struct Settings {
        bool IsEnabled = true;
        Constants Values;
        void Clamp()
        {
            Values.FocusUV.x = std::clamp(Values.FocusUV.x, 0.0f, 1.0f);
            Values.FocusUV.y = std::clamp(Values.FocusUV.y, 0.0f, 1.0f);
            for (float& k : Values.Offsets) k = std::clamp(k, -0.0625f, 0.0625f);
        }
    };

    explicit ChromaticAberration(DeviceContext& deviceContext) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    // SetTextures(input, output): width x height float4 DEVICE buffers; the pass gathers, so output must not overlap input
    void SetTextures(const void* input, void* output, UInt2 size)
    {
        m_input = input;
        m_output = output;
        m_size = size;
    }

    // Process: one launch, asynchronous on the context's stream
    void Process(const Constants& constants)
    {
        PtChromaticAberrationSettings s{};
        s.Size[0] = m_size.x; s.Size[1] = m_size.y;
        s.FocusUV[0] = constants.FocusUV.x; s.FocusUV[1] = constants.FocusUV.y;
        for (int c = 0; c < 3; c++) s.Offsets[c] = constants.Offsets[c];
        const PtChromaticAberrationTextures t{ m_input, m_output };
        ThrowIfFailed(pt_chromatic_aberration(m_ctx, &s, &t), m_ctx, "pt_chromatic_aberration");
    }

private:
    PtContext* m_ctx;
    const void* m_input = nullptr;
    void* m_output = nullptr;
    UInt2 m_size;
};

}  // namespace dxrs::PostProcessing
