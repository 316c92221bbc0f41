// host_upscale.cpp -- drives pt_upscale through the C++ host mirror (dxrs::XeSS) the way the reference's App::Impl does: the render size
// from XeSS::GetInputResolution (SetSuperResolutionOptions), then per frame of a resting camera with Halton jitter the G-buffer
// (LinearDepth, MotionVector) and the radiance at that size, XeSS::SetConstants / Tag / Execute (ProcessXeSSSuperResolution; the first
// frame with Reset, as after m_resetHistory).  Also checks that Execute without an Output tag is refused.  Writes per frame: Jitter
// (2 floats), the inputs it downloaded (Color w*h float4, Depth w*h, Velocity w*h float3) and the output (W*H float4).
// Usage: host_upscale <output width> <output height> <mode 1..5> <frames> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "Raytracing.hpp"
#include "XeSS.hpp"

int main(int argc, char** argv)
{
    if (argc != 6) { std::fprintf(stderr, "usage: %s width height mode frames out.f32\n", argv[0]); return 2; }
    try {
        const uint32_t W = std::atoi(argv[1]), H = std::atoi(argv[2]), mode = std::atoi(argv[3]), frames = std::atoi(argv[4]);
        dxrs::DeviceContext device;
        PtContext* ctx = device.Get();
        dxrs::XeSS xess(device, dxrs::xess_2d_t{ W, H });
        dxrs::xess_2d_t renderSize{};
        if (xess.GetInputResolution(static_cast<dxrs::xess_quality_settings_t>(mode), renderSize) != dxrs::XESS_RESULT_SUCCESS)
            throw std::runtime_error("GetInputResolution failed");
        const uint32_t w = renderSize.x, h = renderSize.y;
        const uint64_t n = (uint64_t)w * h, N = (uint64_t)W * H;
        dxrs::Raytracing raytracing(device);
        dxrs::Scene scene;
        scene.Load(dxrs::MySceneDesc(0));
        raytracing.SetScene(scene);
        dxrs::CameraController controller;
        controller.SetPosition(scene.Desc.Camera.Position);
        controller.SetLens(1.57079632679489661923f, float(w) / float(h), 1e-2f);

        auto alloc = [&](uint64_t bytes) { void* p = nullptr; dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &p), ctx, "pt_device_alloc"); return p; };
        void *depth = alloc(n * 4), *mv = alloc(n * 12), *radiance = alloc(n * 16), *color = alloc(N * 16);
        dxrs::GBufferGeneration gbuffer;
        gbuffer.GPUBuffers.LinearDepth = depth;
        gbuffer.GPUBuffers.MotionVector = mv;
        FILE* f = std::fopen(argv[5], "wb");
        if (!f) throw std::runtime_error("cannot write output");
        dxrs::Camera camera, previous;
        for (uint32_t frame = 0; frame < frames; frame++) {
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
            dxrs::ThrowIfFailed(pt_render(ctx, nullptr, radiance, 1, nullptr), ctx, "pt_render");

            dxrs::XeSSSettings settings;
            settings.InputSize = renderSize;
            settings.Jitter[0] = -camera.Jitter.x;
            settings.Jitter[1] = -camera.Jitter.y;
            settings.Reset = frame == 0;
            xess.SetConstants(settings);
            xess.Tag(dxrs::XeSSResourceType::Depth, depth);
            xess.Tag(dxrs::XeSSResourceType::Velocity, mv);
            xess.Tag(dxrs::XeSSResourceType::Color, radiance);
            xess.Tag(dxrs::XeSSResourceType::Output, color);
            if (xess.Execute() != dxrs::XESS_RESULT_SUCCESS) throw std::runtime_error("XeSS::Execute failed");

            std::vector<float> out(2 + n * 8 + N * 4);
            out[0] = settings.Jitter[0];
            out[1] = settings.Jitter[1];
            dxrs::ThrowIfFailed(pt_download(ctx, radiance, &out[2], n * 16), ctx, "pt_download");
            dxrs::ThrowIfFailed(pt_download(ctx, depth, &out[2 + n * 4], n * 4), ctx, "pt_download");
            dxrs::ThrowIfFailed(pt_download(ctx, mv, &out[2 + n * 5], n * 12), ctx, "pt_download");
            dxrs::ThrowIfFailed(pt_download(ctx, color, &out[2 + n * 8], N * 16), ctx, "pt_download");
            if (std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) throw std::runtime_error("cannot write output");
        }
        std::fclose(f);
        xess.Tag(dxrs::XeSSResourceType::Output, nullptr);
        if (xess.Execute() == dxrs::XESS_RESULT_SUCCESS) throw std::logic_error("a missing Output was accepted");
        std::printf("expected error: %s\n", pt_last_error(ctx));
        for (void* b : { depth, mv, radiance, color }) pt_device_free(ctx, b);
        std::printf("XeSS mode %u: input %ux%u -> %ux%u, %u frames\n", mode, w, h, W, H, frames);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
