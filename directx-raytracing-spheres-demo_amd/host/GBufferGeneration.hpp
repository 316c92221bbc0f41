// GBufferGeneration.hpp -- host mirror of Source/GBufferGeneration.ixx: the pass's `Flags` (GBufferGeneration.hlsl:11-30) and
// its `Textures` (the 13 output textures), bound to pt_render_gbuffer (row N6, DESIGN.md spec S12) instead of a D3D12 dispatch.
// The reference selects channel groups with Flags; here a channel is requested by giving its buffer, so Flags only decide which
// of the bound buffers reach PtGBuffer.
#pragma once

#include "../../include/pt_api.h"

namespace dxrs {

struct GBufferGeneration {
    struct Flags {  // GBufferGeneration.hlsl:11-30
        enum : uint32_t {
            Position = 0x1,
            FlatNormal = 0x2,
            GeometricNormal = 0x4,
            LinearDepth = 0x8,
            NormalizedDepth = 0x10,
            MotionVector = 0x20,
            DiffuseAlbedo = 0x40,
            SpecularAlbedo = 0x80,
            Albedo = DiffuseAlbedo | SpecularAlbedo,
            NormalRoughness = 0x100,
            Radiance = 0x200,
            Geometry = Position | FlatNormal | GeometricNormal | LinearDepth | NormalizedDepth | MotionVector | NormalRoughness,
            Material = 0x400 | Albedo | NormalRoughness | Radiance  // 0x400: BaseColorMetalness, IOR, Transmission
        };
    };

    // device buffers (row-major float32, the channel counts of S12), nullptr = not bound
    struct Textures {
        void *Position{}, *FlatNormal{}, *GeometricNormal{}, *LinearDepth{}, *NormalizedDepth{}, *MotionVector{}, *BaseColorMetalness{},
            *DiffuseAlbedo{}, *SpecularAlbedo{}, *NormalRoughness{}, *IOR{}, *Transmission{}, *Radiance{};
    } GPUBuffers;

    uint32_t RenderFlags = Flags::Geometry | Flags::Material;

    // the PtGBuffer of the bound buffers that RenderFlags selects (GBufferGeneration.hlsl's SET / SET1 conditions)
    PtGBuffer Outputs() const
    {
        const auto pick = [&](void* p, uint32_t flag) { return (RenderFlags & flag) ? p : nullptr; };
        PtGBuffer o{};
        o.Position = pick(GPUBuffers.Position, Flags::Position);
        o.FlatNormal = pick(GPUBuffers.FlatNormal, Flags::FlatNormal);
        o.GeometricNormal = pick(GPUBuffers.GeometricNormal, Flags::GeometricNormal);
        o.LinearDepth = pick(GPUBuffers.LinearDepth, Flags::LinearDepth);
        o.NormalizedDepth = pick(GPUBuffers.NormalizedDepth, Flags::NormalizedDepth);
        o.MotionVector = pick(GPUBuffers.MotionVector, Flags::MotionVector);
        o.BaseColorMetalness = pick(GPUBuffers.BaseColorMetalness, 0x400);
        o.DiffuseAlbedo = pick(GPUBuffers.DiffuseAlbedo, Flags::DiffuseAlbedo);
        o.SpecularAlbedo = pick(GPUBuffers.SpecularAlbedo, Flags::SpecularAlbedo);
        o.NormalRoughness = pick(GPUBuffers.NormalRoughness, Flags::NormalRoughness);
        o.IOR = pick(GPUBuffers.IOR, 0x400);
        o.Transmission = pick(GPUBuffers.Transmission, 0x400);
        o.Radiance = pick(GPUBuffers.Radiance, Flags::Radiance);
        return o;
    }

    // GBufferGeneration::Render (GBufferGeneration.ixx:80-117): the frame the next pt_render renders.  previousSpheres /
    // previousRotations: PreviousObjectToWorld of Scene::Refresh (nullptr = the current pose).
    PtStatus Render(PtContext* context, const PtSphere* previousSpheres = nullptr, const float* previousRotations = nullptr) const
    {
        const PtGBuffer o = Outputs();
        return pt_render_gbuffer(context, nullptr, &o, previousSpheres, previousRotations);
    }

    // The reference's texture formats (Source/App.cpp:431-447; row N27, spec S30): a texel's size, and the Textures read as such textures
    static constexpr uint32_t PackedTexelBytes[13] = { 16, 4, 4, 4, 4, 8, 4, 8, 8, 8, 2, 1, 8 };  // in Textures' order: 79 bytes per pixel
    struct PackedTextures : Textures {};  // the same 13 names; each buffer RenderSize texels of PackedTexelBytes, aligned to its texel

    // Render into textures of the reference's formats (pt_render_gbuffer_packed); RenderFlags select as for Render
    PtStatus Render(PtContext* context, const PackedTextures& textures, const PtSphere* previousSpheres = nullptr, const float* previousRotations = nullptr) const
    {
        GBufferGeneration bound;
        bound.GPUBuffers = textures;
        bound.RenderFlags = RenderFlags;
        const PtGBuffer o = bound.Outputs();
        const PtGBufferPacked q{ o.Position, o.FlatNormal, o.GeometricNormal, o.LinearDepth, o.NormalizedDepth, o.MotionVector, o.BaseColorMetalness,
                                 o.DiffuseAlbedo, o.SpecularAlbedo, o.NormalRoughness, o.IOR, o.Transmission, o.Radiance };
        return pt_render_gbuffer_packed(context, nullptr, &q, previousSpheres, previousRotations);
    }

    // Render with PreviousObjectToWorld taken from the device: the pose published before the newest one (Physics in publishing mode;
    // pt_render_gbuffer_published, row N24)
    PtStatus RenderPublished(PtContext* context) const
    {
        const PtGBuffer o = Outputs();
        return pt_render_gbuffer_published(context, nullptr, &o);
    }
};

}  // namespace dxrs
