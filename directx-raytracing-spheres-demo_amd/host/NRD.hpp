// NRD.hpp -- C++ host mirror of the reference's NRD wrapper (Source/NRD.ixx:88-140: NewFrame, Tag, SetConstants, Denoise) over
// pt_nrd_denoise (row N9, DESIGN.md spec S15), a stand-in for NRD itself, which the reference does not vendor; with
// UseReblurStandIn(true) Identifier::REBLUR goes to pt_nrd_reblur (row N30, spec S32: ReBLUR's own recurrent-blur family).  The nrd:: names
// below are the subset of NRD's API that App::ProcessNRD (Source/App.cpp:1584-1638) uses; resources are DEVICE pointers of
// RenderSize texels (the layouts of PtNrdDenoiseTextures) instead of D3D12 textures.
#pragma once

#include <array>
#include <cstdint>
#include <span>
#include <stdexcept>

#include "Raytracing.hpp"

namespace dxrs {

namespace nrd {

enum class ResourceType : uint32_t {
    IN_MV, IN_NORMAL_ROUGHNESS, IN_VIEWZ, IN_BASECOLOR_METALNESS, IN_DIFF_RADIANCE_HITDIST, IN_SPEC_RADIANCE_HITDIST,
    OUT_DIFF_RADIANCE_HITDIST, OUT_SPEC_RADIANCE_HITDIST, OUT_VALIDATION, MAX_NUM
};
enum class AccumulationMode : uint8_t { CONTINUE, RESTART, CLEAR_AND_RESTART };
enum class HitDistanceReconstructionMode : uint8_t { OFF, AREA_3X3, AREA_5X5 };
// App::ProcessNRD casts its Denoiser to nrd::Identifier: 2 = ReBLUR, 3 = ReLAX
enum class Identifier : uint32_t { REBLUR = static_cast<uint32_t>(Denoiser::NRDReBLUR), RELAX = static_cast<uint32_t>(Denoiser::NRDReLAX) };

struct CommonSettings {            // the fields the stand-in reads (the others App::ProcessNRD fills are accepted by their absence)
    uint16_t rectSize[2]{};
    uint32_t frameIndex{};
    AccumulationMode accumulationMode = AccumulationMode::CONTINUE;
    bool isBaseColorMetalnessAvailable = true;
    bool enableValidation = false;   // OUT_VALIDATION: out of scope, ignored
};

struct ReblurSettings {
    uint32_t maxAccumulatedFrameNum = 30;
    HitDistanceReconstructionMode hitDistanceReconstructionMode = HitDistanceReconstructionMode::OFF;  // the stand-in always uses AREA_3X3
    bool enableAntiFirefly = false;                                                                   // ... and always its anti-firefly
    uint32_t atrousIterationNum = 5;  // (the stand-in's a-trous depth; not an NRD field)
    // read by pt_nrd_reblur only (UseReblurStandIn): nrd::ReblurSettings' defaults as recollected
    uint32_t maxFastAccumulatedFrameNum = 6;
    uint32_t historyFixFrameNum = 3;
    float minBlurRadius = 1.0f;
    float maxBlurRadius = 30.0f;
};

struct RelaxSettings {
    uint32_t diffuseMaxAccumulatedFrameNum = 30;
    uint32_t specularMaxAccumulatedFrameNum = 30;
    HitDistanceReconstructionMode hitDistanceReconstructionMode = HitDistanceReconstructionMode::OFF;
    bool enableAntiFirefly = false;
    uint32_t atrousIterationNum = 5;
};

}  // namespace nrd

class NRD {
public:
    explicit NRD(DeviceContext& deviceContext) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    bool IsAvailable() const { return true; }

    void NewFrame() {}

    // the reference returns false for a texture it cannot wrap; here a null pointer
    bool Tag(nrd::ResourceType type, const void* devicePointer)
    {
        if (type >= nrd::ResourceType::MAX_NUM) return false;
        m_resources[static_cast<size_t>(type)] = devicePointer;
        return devicePointer != nullptr || type == nrd::ResourceType::IN_BASECOLOR_METALNESS;
    }

    // opt-in (default off: REBLUR runs pt_nrd_denoise's filter on ReBLUR's encoding, as before): route Identifier::REBLUR to pt_nrd_reblur
    void UseReblurStandIn(bool on) { m_reblurStandIn = on; }
    bool IsReblurStandInUsed() const { return m_reblurStandIn; }

    bool SetConstants(const nrd::CommonSettings& commonSettings)
    {
        m_common = commonSettings;
        return true;
    }

    bool SetConstants(nrd::Identifier denoiser, const nrd::ReblurSettings& settings)
    {
        if (denoiser != nrd::Identifier::REBLUR) return false;
        m_maxDiffuse = m_maxSpecular = settings.maxAccumulatedFrameNum;
        m_iterations = settings.atrousIterationNum;
        m_reblur = settings;
        return true;
    }

    bool SetConstants(nrd::Identifier denoiser, const nrd::RelaxSettings& settings)
    {
        if (denoiser != nrd::Identifier::RELAX) return false;
        m_maxDiffuse = settings.diffuseMaxAccumulatedFrameNum;
        m_maxSpecular = settings.specularMaxAccumulatedFrameNum;
        m_iterations = settings.atrousIterationNum;
        return true;
    }

    // one pt_nrd_denoise (or pt_nrd_reblur) call per denoiser, asynchronous on the context's stream
    void Denoise(std::span<const nrd::Identifier> denoisers)
    {
        for (const nrd::Identifier denoiser : denoisers) {
            if (m_reblurStandIn && denoiser == nrd::Identifier::REBLUR) {
                DenoiseReblur();
                continue;
            }
            PtNrdDenoiseSettings s{};
            s.RenderSize[0] = m_common.rectSize[0];
            s.RenderSize[1] = m_common.rectSize[1];
            s.Denoiser = static_cast<uint32_t>(denoiser);
            s.AccumulationMode = static_cast<uint32_t>(m_common.accumulationMode);
            s.FrameIndex = m_common.frameIndex;
            s.MaxDiffuseFrames = m_maxDiffuse;
            s.MaxSpecularFrames = m_maxSpecular;
            s.AtrousIterations = m_iterations;
            auto r = [&](nrd::ResourceType t) { return m_resources[static_cast<size_t>(t)]; };
            const PtNrdDenoiseTextures t{r(nrd::ResourceType::IN_VIEWZ), r(nrd::ResourceType::IN_MV), r(nrd::ResourceType::IN_NORMAL_ROUGHNESS),
                                         m_common.isBaseColorMetalnessAvailable ? r(nrd::ResourceType::IN_BASECOLOR_METALNESS) : nullptr,
                                         r(nrd::ResourceType::IN_DIFF_RADIANCE_HITDIST), r(nrd::ResourceType::IN_SPEC_RADIANCE_HITDIST),
                                         const_cast<void*>(r(nrd::ResourceType::OUT_DIFF_RADIANCE_HITDIST)),
                                         const_cast<void*>(r(nrd::ResourceType::OUT_SPEC_RADIANCE_HITDIST))};
            ThrowIfFailed(pt_nrd_denoise(m_ctx, &s, &t), m_ctx, "pt_nrd_denoise");
        }
    }

private:
    void DenoiseReblur()
    {
        PtNrdReblurSettings s{};
        s.RenderSize[0] = m_common.rectSize[0];
        s.RenderSize[1] = m_common.rectSize[1];
        s.AccumulationMode = static_cast<uint32_t>(m_common.accumulationMode);
        s.FrameIndex = m_common.frameIndex;
        s.MaxAccumulatedFrames = m_reblur.maxAccumulatedFrameNum;
        s.MaxFastAccumulatedFrames = m_reblur.maxFastAccumulatedFrameNum;
        s.HistoryFixFrames = m_reblur.historyFixFrameNum;
        s.MinBlurRadius = m_reblur.minBlurRadius;
        s.MaxBlurRadius = m_reblur.maxBlurRadius;
        auto r = [&](nrd::ResourceType t) { return m_resources[static_cast<size_t>(t)]; };
        const PtNrdDenoiseTextures t{r(nrd::ResourceType::IN_VIEWZ), r(nrd::ResourceType::IN_MV), r(nrd::ResourceType::IN_NORMAL_ROUGHNESS),
                                     m_common.isBaseColorMetalnessAvailable ? r(nrd::ResourceType::IN_BASECOLOR_METALNESS) : nullptr,
                                     r(nrd::ResourceType::IN_DIFF_RADIANCE_HITDIST), r(nrd::ResourceType::IN_SPEC_RADIANCE_HITDIST),
                                     const_cast<void*>(r(nrd::ResourceType::OUT_DIFF_RADIANCE_HITDIST)),
                                     const_cast<void*>(r(nrd::ResourceType::OUT_SPEC_RADIANCE_HITDIST))};
        ThrowIfFailed(pt_nrd_reblur(m_ctx, &s, &t), m_ctx, "pt_nrd_reblur");
    }

    PtContext* m_ctx;
    std::array<const void*, static_cast<size_t>(nrd::ResourceType::MAX_NUM)> m_resources{};
    nrd::CommonSettings m_common{};
    uint32_t m_maxDiffuse = 30, m_maxSpecular = 30, m_iterations = 5;
    nrd::ReblurSettings m_reblur{};
    bool m_reblurStandIn = false;
};

}  // namespace dxrs
