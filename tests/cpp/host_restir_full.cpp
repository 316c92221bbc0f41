// host_restir_full.cpp -- drives pt_restir_di_full through the C++ host mirror (dxrs::RTXDI) the way the reference's App::Impl::Render
// does (Source/App.cpp:1187-1227): the SetConstants overload that takes ShadingSettings, with Pairwise bias correction in both reuse
// passes and final-visibility reuse at the mirror's defaults (4 frames, 16 pixels) turned on, for a few frames of a resting camera over
// the demo scene.  Also checks that the older SetConstants overload keeps refusing Pairwise, and that the refusal names the entry point
// that accepts it.  Writes per frame what host_restir_di_ex.cpp writes: the camera's Position and PreviousPosition (6 floats), the
// Diffuse / Specular buffers as they were before the pass, the eight G-buffer inputs and the Diffuse / Specular buffers after the pass.
// Usage: host_restir_full <width> <height> <frames> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "RTXDI.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s width height frames out.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]), frames = std::atoi(argv[3]);
        const uint64_t n = (uint64_t)w * h;
        dxrs::DeviceContext device;
        PtContext* ctx = device.Get();
        dxrs::Raytracing raytracing(device);
        dxrs::Scene scene;
        scene.Load(dxrs::MySceneDesc(0));
        raytracing.SetScene(scene);
        dxrs::CameraController controller;
        controller.SetPosition(scene.Desc.Camera.Position);
        controller.SetLens(1.57079632679489661923f, float(w) / float(h));

        auto alloc = [&](uint64_t bytes) { void* p = nullptr; dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &p), ctx, "pt_device_alloc"); return p; };
        const uint32_t widths[10] = { 4, 2, 1, 3, 4, 4, 1, 1, 4, 4 };
        void* buffers[10];
        for (int k = 0; k < 10; k++) buffers[k] = alloc(n * 4 * widths[k]);
        dxrs::GBufferGeneration gbuffer;
        gbuffer.GPUBuffers.Position = buffers[0];
        gbuffer.GPUBuffers.GeometricNormal = buffers[1];
        gbuffer.GPUBuffers.LinearDepth = buffers[2];
        gbuffer.GPUBuffers.MotionVector = buffers[3];
        gbuffer.GPUBuffers.BaseColorMetalness = buffers[4];
        gbuffer.GPUBuffers.NormalRoughness = buffers[5];
        gbuffer.GPUBuffers.IOR = buffers[6];
        gbuffer.GPUBuffers.Transmission = buffers[7];
        dxrs::RTXDI rtxdi(device);
        rtxdi.GPUBuffers = { buffers[0], buffers[1], buffers[2], buffers[3], buffers[4], buffers[5], buffers[6], buffers[7], buffers[8], buffers[9] };
        dxrs::ReSTIRDISettings settings;
        settings.TemporalResampling.BiasCorrectionMode = dxrs::ReSTIRDI_BiasCorrectionMode::Pairwise;
        settings.SpatialResampling.BiasCorrectionMode = dxrs::ReSTIRDI_BiasCorrectionMode::Pairwise;
        settings.SpatialResampling.Samples = 2;
        dxrs::ShadingSettings shading;
        shading.ReuseFinalVisibility = true;
        dxrs::Camera camera;
        FILE* f = std::fopen(argv[4], "wb");
        if (!f) throw std::runtime_error("cannot write output");
        for (uint32_t frame = 0; frame < frames; frame++) {
            const dxrs::Camera previous = camera;
            controller.Fill(camera, dxrs::Float2{});
            if (frame == 0) controller.FillMatrices(camera);  // a first frame: the Previous* matrices are this frame's own
            else controller.FillMatrices(camera, previous);
            raytracing.SetCamera(camera);
            {
                const PtCamera c = dxrs::ToPt(camera);
                const float pos[6] = { c.Position[0], c.Position[1], c.Position[2], c.PreviousPosition[0], c.PreviousPosition[1], c.PreviousPosition[2] };
                if (std::fwrite(pos, sizeof(float), 6, f) != 6) throw std::runtime_error("cannot write output");
            }
            dxrs::Raytracing::GraphicsSettings gs;
            gs.RenderSize = { w, h }; gs.FrameIndex = frame; gs.Bounces = 8; gs.SamplesPerPixel = 1; gs.IsRussianRouletteEnabled = true;
            raytracing.SetConstants(gs);
            raytracing.UploadConstants();
            // known content for the two outputs: an ordinary frame, downloaded before the pass (see host_restir_di_ex.cpp)
            for (int k = 8; k < 10; k++) {
                dxrs::ThrowIfFailed(pt_render(ctx, nullptr, buffers[k], 1, nullptr), ctx, "pt_render");
                std::vector<float> c(n * 4);
                dxrs::ThrowIfFailed(pt_download(ctx, buffers[k], c.data(), c.size() * 4), ctx, "pt_download");
                if (std::fwrite(c.data(), sizeof(float), c.size(), f) != c.size()) throw std::runtime_error("cannot write output");
            }
            dxrs::ThrowIfFailed(gbuffer.Render(ctx), ctx, "GBufferGeneration::Render");
            rtxdi.SetConstants(settings, shading, frame == 0, { w, h }, frame);
            rtxdi.Render();
            for (int k = 0; k < 10; k++) {
                std::vector<float> c(n * widths[k]);
                dxrs::ThrowIfFailed(pt_download(ctx, buffers[k], c.data(), c.size() * 4), ctx, "pt_download");
                if (std::fwrite(c.data(), sizeof(float), c.size(), f) != c.size()) throw std::runtime_error("cannot write output");
            }
        }
        std::fclose(f);
        try {
            rtxdi.SetConstants(settings, false, { w, h }, frames);  // the overload without ShadingSettings: the present route
            rtxdi.Render();
            throw std::logic_error("pairwise bias correction was accepted by the old overload");
        } catch (const std::runtime_error& e) {
            std::printf("expected error: %s\n", e.what());
        }
        for (void* b : buffers) pt_device_free(ctx, b);
        std::printf("ReSTIR DI with pairwise MIS and final-visibility reuse: %ux%u, %u frames\n", w, h, frames);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
