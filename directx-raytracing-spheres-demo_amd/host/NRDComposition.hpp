// NRDComposition.hpp -- C++ host mirror of PostProcessing::NRDComposition (Source/NRDComposition.ixx): the pass object the reference's
// App::Impl::ProcessNRD (Source/App.cpp:1549-1642) runs once with Pack = true before NRD and once with Pack = false after it, over
// pt_nrd_composition (row N8, DESIGN.md spec S14).
#pragma once

#include <stdexcept>

#include "Raytracing.hpp"

namespace dxrs::PostProcessing {

struct NRDComposition {
    // NRDComposition::Constants (byte-identical: PtNrdCompositionConstants, 32 B)
    struct Constants {
        UInt2 RenderSize;
        uint32_t Pack;
        dxrs::Denoiser Denoiser;
        Float4 ReBLURHitDistance;
    };
    static_assert(sizeof(Constants) == sizeof(PtNrdCompositionConstants), "NRDComposition::Constants layout");

    // nrd::ReblurSettings().hitDistanceParameters, what App::ProcessNRD passes in ReBLURHitDistance
    static constexpr Float4 DefaultReBLURHitDistance{3.0f, 0.1f, 20.0f, -25.0f};

    // NRDComposition::Textures: DEVICE buffers of RenderSize texels (the layouts of PtNrdCompositionTextures)
    struct {
        const void *LinearDepth, *DiffuseAlbedo, *SpecularAlbedo, *NormalRoughness;
        void *NoisyDiffuse, *NoisySpecular;
        const void *DenoisedDiffuse, *DenoisedSpecular;
        void* Radiance;
    } Textures{};

    explicit NRDComposition(DeviceContext& deviceContext) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    // Process: pack (constants.Pack != 0) or compose, asynchronous on the context's stream
    void Process(const Constants& constants)
    {
        PtNrdCompositionConstants k{};
        k.RenderSize[0] = constants.RenderSize.x;
        k.RenderSize[1] = constants.RenderSize.y;
        k.Pack = constants.Pack;
        k.Denoiser = static_cast<uint32_t>(constants.Denoiser);
        k.ReBLURHitDistance[0] = constants.ReBLURHitDistance.x;
        k.ReBLURHitDistance[1] = constants.ReBLURHitDistance.y;
        k.ReBLURHitDistance[2] = constants.ReBLURHitDistance.z;
        k.ReBLURHitDistance[3] = constants.ReBLURHitDistance.w;
        const PtNrdCompositionTextures t{Textures.LinearDepth, Textures.DiffuseAlbedo, Textures.SpecularAlbedo, Textures.NormalRoughness,
                                         Textures.NoisyDiffuse, Textures.NoisySpecular, Textures.DenoisedDiffuse, Textures.DenoisedSpecular,
                                         Textures.Radiance};
        ThrowIfFailed(pt_nrd_composition(m_ctx, &k, &t), m_ctx, "pt_nrd_composition");
    }

private:
    PtContext* m_ctx;
};

}  // namespace dxrs::PostProcessing
