// host_rr.cpp -- drives pt_ray_reconstruction through the C++ host mirror (dxrs::RayReconstruction) the way the reference's App::Impl
// does with Denoiser::DLSSRayReconstruction selected: per frame of a travelling camera with Halton jitter the G-buffer (LinearDepth,
// MotionVector, NormalRoughness, DiffuseAlbedo, SpecularAlbedo) and the denoiser frame of mode 1 (radiance + SpecularHitDistance) at
// render size, then SetConstants / Tag / Evaluate (ProcessDLSSRayReconstruction).  Also checks that Evaluate without an output tag
// calls nothing, and that the library refuses a null Output.  Writes per frame: Jitter (2 floats), Position (3), ProjectionToView,
// ViewToWorld, PreviousWorldToProjection (16 each), the inputs it downloaded (Color w*h float4, Depth w*h, MotionVector w*h float3,
// NormalRoughness w*h float4, DiffuseAlbedo and SpecularAlbedo w*h float3, SpecularHitDistance w*h) and the output (W*H float4).
// Usage: host_rr <render width> <render height> <output width> <output height> <frames> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "RayReconstruction.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: %s w h W H frames out.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]), W = std::atoi(argv[3]), H = std::atoi(argv[4]), frames = std::atoi(argv[5]);
        const uint64_t n = (uint64_t)w * h, N = (uint64_t)W * H;
        dxrs::DeviceContext device;
        PtContext* ctx = device.Get();
        dxrs::Raytracing raytracing(device);
        dxrs::Scene scene;
        scene.Load(dxrs::MySceneDesc(0));
        raytracing.SetScene(scene);
        dxrs::CameraController controller;
        controller.SetLens(1.57079632679489661923f, float(w) / float(h), 1e-2f);

        auto alloc = [&](uint64_t bytes) { void* p = nullptr; dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &p), ctx, "pt_device_alloc"); return p; };
        void *radiance = alloc(n * 16), *depth = alloc(n * 4), *mv = alloc(n * 12), *nr = alloc(n * 16), *da = alloc(n * 12), *sa = alloc(n * 12),
             *hit = alloc(n * 4), *color = alloc(N * 16);  // (texels of SpecularHitDistance the frame leaves alone reach the stand-in and the file alike)
        dxrs::GBufferGeneration gbuffer;
        gbuffer.GPUBuffers.LinearDepth = depth;
        gbuffer.GPUBuffers.MotionVector = mv;
        gbuffer.GPUBuffers.NormalRoughness = nr;
        gbuffer.GPUBuffers.DiffuseAlbedo = da;
        gbuffer.GPUBuffers.SpecularAlbedo = sa;
        dxrs::RayReconstruction rr(device, { W, H });
        using Type = dxrs::RayReconstruction::BufferType;
        FILE* f = std::fopen(argv[6], "wb");
        if (!f) throw std::runtime_error("cannot write output");
        dxrs::Camera camera, previous;
        for (uint32_t frame = 0; frame < frames; frame++) {
            dxrs::Float3 position = scene.Desc.Camera.Position;
            position.x += 0.15f * float(frame);
            position.z += 0.1f * float(frame);
            controller.SetPosition(position);
            const auto halton = dxrs::HaltonSampler::Get2D(frame % 32 + 1);
            controller.Fill(camera, dxrs::Float2{ halton.x - 0.5f, halton.y - 0.5f });
            if (frame == 0) controller.FillMatrices(camera);
            else controller.FillMatrices(camera, previous);
            previous = camera;
            raytracing.SetCamera(camera);
            dxrs::Raytracing::GraphicsSettings gs;
            gs.RenderSize = { w, h }; gs.FrameIndex = frame; gs.Bounces = 8; gs.SamplesPerPixel = 1; gs.IsRussianRouletteEnabled = true;
            raytracing.SetConstants(gs);
            raytracing.UploadConstants();
            dxrs::ThrowIfFailed(gbuffer.Render(ctx), ctx, "GBufferGeneration::Render");
            PtDenoiserOutputs outputs{};
            outputs.Denoiser = 1;  // Denoiser::DLSSRayReconstruction
            outputs.SpecularHitDistance = hit;
            dxrs::ThrowIfFailed(pt_render_denoiser(ctx, nullptr, radiance, 1, &outputs, nullptr), ctx, "pt_render_denoiser");

            rr.SetConstants(camera, { w, h });
            rr.Tag(Type::ScalingInputColor, radiance);
            rr.Tag(Type::Depth, depth);
            rr.Tag(Type::MotionVectors, mv);
            rr.Tag(Type::NormalRoughness, nr);
            rr.Tag(Type::Albedo, da);
            rr.Tag(Type::SpecularAlbedo, sa);
            rr.Tag(Type::SpecularHitDistance, hit);
            rr.Tag(Type::ScalingOutputColor, color);
            if (rr.Evaluate() != dxrs::RayReconstruction::Result::eOk) throw std::runtime_error("RayReconstruction::Evaluate failed");

            std::vector<float> out(53 + n * 19 + N * 4);
            out[0] = -camera.Jitter.x;
            out[1] = -camera.Jitter.y;
            out[2] = camera.Position.x; out[3] = camera.Position.y; out[4] = camera.Position.z;
            for (int k = 0; k < 16; k++) { out[5 + k] = camera.Matrices[6][k]; out[21 + k] = camera.Matrices[7][k]; out[37 + k] = camera.Matrices[2][k]; }
            size_t o = 53;
            const struct { const void* p; uint64_t floats; } parts[] = { { radiance, n * 4 }, { depth, n }, { mv, n * 3 }, { nr, n * 4 }, { da, n * 3 }, { sa, n * 3 },
                                                                        { hit, n }, { color, N * 4 } };
            for (const auto& part : parts) {
                dxrs::ThrowIfFailed(pt_download(ctx, part.p, &out[o], part.floats * 4), ctx, "pt_download");
                o += part.floats;
            }
            if (std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) throw std::runtime_error("cannot write output");
        }
        std::fclose(f);
        rr.Tag(Type::ScalingOutputColor, nullptr);
        if (rr.Evaluate() != dxrs::RayReconstruction::Result::eErrorMissingInputParameter) throw std::logic_error("a missing output tag was accepted");
        PtRayReconstructionSettings s{};
        s.RenderSize[0] = w; s.RenderSize[1] = h; s.OutputSize[0] = W; s.OutputSize[1] = H;
        const PtRayReconstructionTextures t{ radiance, depth, mv, nr, da, sa, hit, nullptr };
        if (pt_ray_reconstruction(ctx, &s, &t) != PT_ERR_INVALID_ARG) throw std::logic_error("a null Output was accepted");
        std::printf("expected error: %s\n", pt_last_error(ctx));
        for (void* b : { radiance, depth, mv, nr, da, sa, hit, color }) pt_device_free(ctx, b);
        std::printf("ray reconstruction: %ux%u -> %ux%u, %u frames\n", w, h, W, H, frames);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
