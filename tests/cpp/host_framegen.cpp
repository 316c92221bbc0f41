// host_framegen.cpp -- drives pt_frame_gen through the C++ host mirror (dxrs::FrameGeneration) the way the reference's App::Impl ends
// PostProcessGraphics: per frame of a travelling camera the G-buffer (LinearDepth, MotionVector), the radiance, the tone map, then
// ProcessDLSSFrameGeneration's three tags and the generated frame.  Also checks that the feature switched off queues nothing, and that a
// missing tag and an output that is the tagged colour are refused.  Writes per frame: generated (uint32), the inputs it downloaded
// (Color w*h uint32, Depth w*h float, MotionVector w*h float3) and the output (w*h uint32).
// Usage: host_framegen <width> <height> <frames> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "FrameGeneration.hpp"
#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s width height frames out.bin\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]), frames = std::atoi(argv[3]);
        const uint64_t n = (uint64_t)w * h;
        dxrs::DeviceContext device;
        PtContext* ctx = device.Get();
        dxrs::FrameGeneration frameGeneration(device);
        dxrs::Raytracing raytracing(device);
        dxrs::Scene scene;
        scene.Load(dxrs::MySceneDesc(0));
        raytracing.SetScene(scene);
        dxrs::CameraController controller;
        controller.SetLens(1.57079632679489661923f, float(w) / float(h), 1e-2f);

        auto alloc = [&](uint64_t bytes) { void* p = nullptr; dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &p), ctx, "pt_device_alloc"); return p; };
        void *depth = alloc(n * 4), *mv = alloc(n * 12), *radiance = alloc(n * 16), *color = alloc(n * 4), *generatedFrame = alloc(n * 4);
        dxrs::GBufferGeneration gbuffer;
        gbuffer.GPUBuffers.LinearDepth = depth;
        gbuffer.GPUBuffers.MotionVector = mv;
        PtToneMapParams tone{};
        tone.Operator = 3; tone.TransferFunction = 1; tone.LinearExposure = 1.0f; tone.PaperWhiteNits = 200.0f;

        using FG = dxrs::FrameGeneration;
        bool generated = true;
        // off: nothing is called, even without tags
        if (frameGeneration.Generate({ w, h }, { w, h }, generatedFrame, generated) != FG::Result::eOk || generated) throw std::logic_error("eOff generated a frame");
        frameGeneration.SetOptions(dxrs::sl::DLSSGMode::eOn);

        FILE* f = std::fopen(argv[4], "wb");
        if (!f) throw std::runtime_error("cannot write output");
        dxrs::Camera camera, previous;
        for (uint32_t frame = 0; frame < frames; frame++) {
            dxrs::Float3 position = scene.Desc.Camera.Position;
            position.x += 0.25f * float(frame);
            position.y += 0.1f * float(frame);
            controller.SetPosition(position);
            controller.Fill(camera, dxrs::Float2{ 0.0f, 0.0f });
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
            dxrs::ThrowIfFailed(pt_tonemap(ctx, radiance, (uint32_t)n, &tone, color), ctx, "pt_tonemap");

            // App::ProcessDLSSFrameGeneration
            frameGeneration.Tag(FG::BufferType::Depth, depth);
            frameGeneration.Tag(FG::BufferType::MotionVectors, mv);
            frameGeneration.Tag(FG::BufferType::HUDLessColor, color);
            if (frameGeneration.Generate({ w, h }, { w, h }, generatedFrame, generated) != FG::Result::eOk) throw std::runtime_error("FrameGeneration::Generate failed");

            std::vector<uint32_t> out(1 + n * 6);
            out[0] = generated ? 1u : 0u;
            dxrs::ThrowIfFailed(pt_download(ctx, color, &out[1], n * 4), ctx, "pt_download");
            dxrs::ThrowIfFailed(pt_download(ctx, depth, &out[1 + n], n * 4), ctx, "pt_download");
            dxrs::ThrowIfFailed(pt_download(ctx, mv, &out[1 + 2 * n], n * 12), ctx, "pt_download");
            dxrs::ThrowIfFailed(pt_download(ctx, generatedFrame, &out[1 + 5 * n], n * 4), ctx, "pt_download");
            if (std::fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size()) throw std::runtime_error("cannot write output");
        }
        std::fclose(f);
        if (frameGeneration.Generate({ w, h }, { w, h }, color, generated) != FG::Result::eErrorInvalidParameter)
            throw std::logic_error("an output that is the tagged colour was not refused");
        std::printf("expected error: %s\n", pt_last_error(ctx));
        frameGeneration.Tag(FG::BufferType::MotionVectors, nullptr);
        if (frameGeneration.Generate({ w, h }, { w, h }, generatedFrame, generated) != FG::Result::eErrorMissingInputParameter)
            throw std::logic_error("a missing tag was not refused");
        std::printf("expected error: missing motion vector tag\n");
        for (void* b : { depth, mv, radiance, color, generatedFrame }) pt_device_free(ctx, b);
        std::printf("frame generation %ux%u, %u frames\n", w, h, frames);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
