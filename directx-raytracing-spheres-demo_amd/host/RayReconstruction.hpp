// RayReconstruction.hpp -- C++ host mirror of what the reference does for DLSS ray reconstruction (App::SetSuperResolutionOptions ->
// slDLSSDSetOptions, App::ProcessDLSSRayReconstruction's tags, constants and Evaluate, Source/App.cpp:1654-1671) over
// pt_ray_reconstruction (row N15, DESIGN.md spec S21), a stand-in for Streamline's DLSS-RR plugin, which the reference does not vendor.
// Resources are DEVICE pointers (the layouts of PtRayReconstructionTextures) instead of D3D12 textures; the camera travels by value
// (Position, ProjectionToView, ViewToWorld, PreviousWorldToProjection of the frame's Camera) in place of sl::Constants and
// DLSSDOptions' worldToCameraView / cameraViewToWorld.  host/Streamline.hpp keeps reporting DLSS_RR as unavailable: this class is the
// stand-in's own interface.
// Not built: presets, exposure, the transparency and particle layer tags.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>

#include "Camera.hpp"
#include "Raytracing.hpp"

namespace dxrs {

class RayReconstruction {
public:
    // the sl::BufferType tags ProcessDLSSRayReconstruction sets, in the order of PtRayReconstructionTextures
    enum class BufferType : uint32_t { ScalingInputColor, Depth, MotionVectors, NormalRoughness, Albedo, SpecularAlbedo, SpecularHitDistance, ScalingOutputColor, Count };
    enum class Result : int32_t { eOk = 0, eErrorInvalidParameter = -1, eErrorMissingInputParameter = -3 };
    struct Extent { uint32_t width, height; };

    RayReconstruction(DeviceContext& deviceContext, Extent outputExtent) : m_ctx(deviceContext.Get()), m_outputExtent(outputExtent)
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
    }

    void ResetHistory() { m_reset = true; }
    // the history cap of the stand-in (not an SDK call): 0 = the library's default
    void SetMaxHistoryWeight(float weight) { m_maxHistoryWeight = weight; }
    void Tag(BufferType type, const void* devicePointer) { m_resources[static_cast<size_t>(type)] = devicePointer; }

    // sl::Constants + DLSSDOptions: the frame's camera, as Raytracing::SetCamera took it; jitterOffset = -camera.Jitter
    void SetConstants(const Camera& camera, Extent renderExtent)
    {
        m_renderExtent = renderExtent;
        m_camera = camera;
    }

    // Streamline::Evaluate(kFeatureDLSS_RR): one pt_ray_reconstruction call, asynchronous on the context's stream
    Result Evaluate()
    {
        PtRayReconstructionSettings s{};
        s.RenderSize[0] = m_renderExtent.width; s.RenderSize[1] = m_renderExtent.height;
        s.OutputSize[0] = m_outputExtent.width; s.OutputSize[1] = m_outputExtent.height;
        s.Jitter[0] = -m_camera.Jitter.x; s.Jitter[1] = -m_camera.Jitter.y;
        s.Reset = m_reset ? 1u : 0u;
        s.MaxHistoryWeight = m_maxHistoryWeight;
        s.Position[0] = m_camera.Position.x; s.Position[1] = m_camera.Position.y; s.Position[2] = m_camera.Position.z;
        std::memcpy(s.ProjectionToView, m_camera.Matrices[6], sizeof s.ProjectionToView);
        std::memcpy(s.ViewToWorld, m_camera.Matrices[7], sizeof s.ViewToWorld);
        std::memcpy(s.PreviousWorldToProjection, m_camera.Matrices[2], sizeof s.PreviousWorldToProjection);
        auto r = [&](BufferType t) { return m_resources[static_cast<size_t>(t)]; };
        const PtRayReconstructionTextures t{ r(BufferType::ScalingInputColor), r(BufferType::Depth), r(BufferType::MotionVectors), r(BufferType::NormalRoughness),
                                             r(BufferType::Albedo), r(BufferType::SpecularAlbedo), r(BufferType::SpecularHitDistance),
                                             const_cast<void*>(r(BufferType::ScalingOutputColor)) };
        for (const void* p : m_resources)
            if (!p) return Result::eErrorMissingInputParameter;  // a tag is missing: nothing is called
        const PtStatus st = pt_ray_reconstruction(m_ctx, &s, &t);
        if (st == PT_ERR_INVALID_ARG) return Result::eErrorInvalidParameter;
        ThrowIfFailed(st, m_ctx, "pt_ray_reconstruction");
        m_reset = false;
        return Result::eOk;
    }

private:
    PtContext* m_ctx;
    Extent m_outputExtent;
    Extent m_renderExtent{};
    Camera m_camera{};
    std::array<const void*, static_cast<size_t>(BufferType::Count)> m_resources{};
    bool m_reset = true;  // the first frame restarts, as after the reference's m_resetHistory
    float m_maxHistoryWeight = 0.0f;
};

}  // namespace dxrs
