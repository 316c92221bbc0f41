// host_chromab.cpp -- drives pt_chromatic_aberration through the C++ host mirror (PostProcessing::ChromaticAberration), against pt_api.h
// alone: render the demo scene into a device buffer, run the pass with the given constants (or the defaults), then write the radiance
// and the result.  An in-place call must be refused.
// Usage: host_chromab <width> <height> <out.f32> [focus_u focus_v k_r k_g k_b]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ChromaticAberration.hpp"
#include "MyScene.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 4 && argc != 9) { std::fprintf(stderr, "usage: %s width height out.f32 [focus_u focus_v k_r k_g k_b]\n", argv[0]); return 2; }
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
        void *radiance = nullptr, *fringed = nullptr;
        dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &radiance), ctx, "pt_device_alloc");
        dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &fringed), ctx, "pt_device_alloc");
        dxrs::ThrowIfFailed(pt_render(ctx, nullptr, radiance, 1, nullptr), ctx, "pt_render");

        dxrs::PostProcessing::ChromaticAberration::Settings settings;  // the defaults
        settings.Values.Offsets[0] = 7.0f; settings.Values.FocusUV.y = -3.0f;
        settings.Clamp();
        if (settings.Values.Offsets[0] != 0.0625f || settings.Values.FocusUV.y != 0.0f) throw std::runtime_error("Clamp");
        settings = {};
        if (argc == 9) {
            settings.Values.FocusUV = { (float)std::atof(argv[4]), (float)std::atof(argv[5]) };
            for (int c = 0; c < 3; c++) settings.Values.Offsets[c] = (float)std::atof(argv[6 + c]);
        }
        dxrs::PostProcessing::ChromaticAberration pass(device);
        if (settings.IsEnabled) {
            pass.SetTextures(radiance, fringed, {w, h});
            pass.Process(settings.Values);
        }
        try {
            pass.SetTextures(radiance, radiance, {w, h});
            pass.Process(settings.Values);
            throw std::logic_error("an in-place call was accepted");
        } catch (const std::runtime_error& e) {
            std::printf("expected error: %s\n", e.what());
        }
        std::vector<float> a((size_t)w * h * 4), b(a.size());
        dxrs::ThrowIfFailed(pt_download(ctx, radiance, a.data(), bytes), ctx, "pt_download");
        dxrs::ThrowIfFailed(pt_download(ctx, fringed, b.data(), bytes), ctx, "pt_download");
        FILE* f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(a.data(), sizeof(float), a.size(), f) != a.size() || std::fwrite(b.data(), sizeof(float), b.size(), f) != b.size())
            throw std::runtime_error("cannot write output");
        std::fclose(f);
        pt_device_free(ctx, radiance);
        pt_device_free(ctx, fringed);
        std::printf("chromatic aberration %ux%u focus %g %g offsets %g %g %g\n", w, h, settings.Values.FocusUV.x, settings.Values.FocusUV.y,
                    settings.Values.Offsets[0], settings.Values.Offsets[1], settings.Values.Offsets[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
