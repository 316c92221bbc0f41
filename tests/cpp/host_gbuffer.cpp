// host_gbuffer.cpp -- drives pt_render_gbuffer through the C++ host mirror (GBufferGeneration, CameraController::FillMatrices) the way
// the reference's App::Impl::Render does before ray tracing: the camera with its matrices, then the G-buffer pass with all channels
// bound, then the frame.  Writes the 13 channels interleaved, 32 floats per pixel in PtGBuffer's order.
// Usage: host_gbuffer <width> <height> <gbuffer.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s width height gbuffer.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]);
        const uint32_t widths[13] = { 4, 2, 2, 1, 1, 3, 4, 3, 3, 4, 1, 1, 3 };
        dxrs::DeviceContext device;
        PtContext* ctx = device.Get();
        dxrs::Raytracing raytracing(device);
        dxrs::Scene scene;
        scene.Load(dxrs::MySceneDesc(0));
        raytracing.SetScene(scene);
        dxrs::CameraController controller;
        controller.SetPosition(scene.Desc.Camera.Position);
        controller.SetLens(1.57079632679489661923f, float(w) / float(h));
        dxrs::Camera camera;
        controller.Fill(camera, dxrs::Float2{});
        camera.PreviousPosition = camera.Position;
        controller.FillMatrices(camera);  // a first frame: the Previous* matrices are this frame's own
        raytracing.SetCamera(camera);
        dxrs::Raytracing::GraphicsSettings gs;
        gs.RenderSize = { w, h }; gs.Bounces = 8; gs.SamplesPerPixel = 1; gs.IsRussianRouletteEnabled = true;
        raytracing.SetConstants(gs);
        raytracing.UploadConstants();

        dxrs::GBufferGeneration gbuffer;
        void* buffers[13] = {};
        for (int k = 0; k < 13; k++) dxrs::ThrowIfFailed(pt_device_alloc(ctx, (uint64_t)w * h * widths[k] * 4, &buffers[k]), ctx, "pt_device_alloc");
        auto& t = gbuffer.GPUBuffers;
        void** slots[13] = { &t.Position, &t.FlatNormal, &t.GeometricNormal, &t.LinearDepth, &t.NormalizedDepth, &t.MotionVector, &t.BaseColorMetalness,
                             &t.DiffuseAlbedo, &t.SpecularAlbedo, &t.NormalRoughness, &t.IOR, &t.Transmission, &t.Radiance };
        for (int k = 0; k < 13; k++) *slots[k] = buffers[k];
        dxrs::ThrowIfFailed(gbuffer.Render(ctx), ctx, "GBufferGeneration::Render");
        void* radiance = nullptr;
        dxrs::ThrowIfFailed(pt_device_alloc(ctx, (uint64_t)w * h * 16, &radiance), ctx, "pt_device_alloc");
        dxrs::ThrowIfFailed(pt_render(ctx, nullptr, radiance, 1, nullptr), ctx, "pt_render");  // the frame, after its G-buffer

        std::vector<float> out((size_t)w * h * 32, 0.0f);
        uint32_t at = 0;
        for (int k = 0; k < 13; k++) {
            std::vector<float> c((size_t)w * h * widths[k]);
            dxrs::ThrowIfFailed(pt_download(ctx, buffers[k], c.data(), c.size() * 4), ctx, "pt_download");
            for (size_t i = 0; i < (size_t)w * h; i++)
                for (uint32_t j = 0; j < widths[k]; j++) out[i * 32 + at + j] = c[i * widths[k] + j];
            at += widths[k];
        }
        FILE* f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) throw std::runtime_error("cannot write output");
        std::fclose(f);
        for (void* b : buffers) pt_device_free(ctx, b);
        pt_device_free(ctx, radiance);
        std::printf("gbuffer %ux%u\n", w, h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
