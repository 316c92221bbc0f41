// host_bloom.cpp -- drives pt_bloom through the C++ host mirror (PostProcessing::Bloom) the way the reference's
// App::Impl::PostProcessGraphics does: render the demo scene into a device buffer, bloom it with the default settings, then
// write the radiance and the bloomed image.
// Usage: host_bloom <width> <height> <radiance.f32> <bloomed.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Bloom.hpp"
#include "MyScene.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s width height radiance.f32 bloomed.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]);
        const uint64_t bytes = (uint64_t)w * h * 16;
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
        raytracing.SetCamera(camera);
        dxrs::Raytracing::GraphicsSettings gs;
        gs.RenderSize = { w, h }; gs.Bounces = 8; gs.SamplesPerPixel = 1; gs.IsRussianRouletteEnabled = true;
        raytracing.SetConstants(gs);
        raytracing.UploadConstants();
        void *radiance = nullptr, *bloomed = nullptr;
        dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &radiance), ctx, "pt_device_alloc");
        dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &bloomed), ctx, "pt_device_alloc");
        dxrs::ThrowIfFailed(pt_render(ctx, nullptr, radiance, 1, nullptr), ctx, "pt_render");

        dxrs::PostProcessing::Bloom::Settings settings;  // the reference's defaults
        settings.Strength = 7.0f;
        settings.Clamp();
        if (settings.Strength != 1.0f) throw std::runtime_error("Strength clamp");
        settings = {};
        dxrs::PostProcessing::Bloom bloom(device);
        if (settings.IsEnabled) {
            bloom.SetTextures(radiance, bloomed, {w, h});
            bloom.Process({settings.Strength});
        }
        try {
            bloom.SetTextures(radiance, bloomed, {16, 16});
            bloom.Process({settings.Strength});
            throw std::logic_error("a 16x16 bloom was accepted");
        } catch (const std::runtime_error& e) {
            std::printf("expected error: %s\n", e.what());
        }
        std::vector<float> a((size_t)w * h * 4), b(a.size());
        dxrs::ThrowIfFailed(pt_download(ctx, radiance, a.data(), bytes), ctx, "pt_download");
        dxrs::ThrowIfFailed(pt_download(ctx, bloomed, b.data(), bytes), ctx, "pt_download");
        for (auto [path, v] : {std::pair{argv[3], &a}, std::pair{argv[4], &b}}) {
            FILE* f = std::fopen(path, "wb");
            if (!f || std::fwrite(v->data(), sizeof(float), v->size(), f) != v->size()) throw std::runtime_error("cannot write output");
            std::fclose(f);
        }
        pt_device_free(ctx, radiance);
        pt_device_free(ctx, bloomed);
        std::printf("bloom %ux%u strength %g\n", w, h, settings.Strength);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
