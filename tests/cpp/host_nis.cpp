// host_nis.cpp -- drives pt_nis_sharpen through the C++ host mirror (dxrs::Streamline) the way the reference's App::ProcessNIS does:
// one frame of the demo scene rendered at the given size, NISOptions{eSharpen, sharpness} set, the radiance tagged as
// ScalingInputColor and a second buffer as ScalingOutputColor, kFeatureNIS evaluated.  Also checks that the DLSS features are reported
// as unavailable and that Evaluate without an output tag, and with the input tagged as the output, is refused.  Writes the radiance (w*h float4), then the sharpened frame.
// Usage: host_nis <width> <height> <sharpness> <hdr mode 0|1> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "MyScene.hpp"
#include "Raytracing.hpp"
#include "Streamline.hpp"

int main(int argc, char** argv)
{
    if (argc != 6) { std::fprintf(stderr, "usage: %s width height sharpness hdr out.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]), hdr = std::atoi(argv[4]);
        const float sharpness = (float)std::atof(argv[3]);
        const uint64_t n = (uint64_t)w * h;
        dxrs::DeviceContext device;
        PtContext* ctx = device.Get();
        dxrs::Streamline streamline(device);
        if (!streamline.IsAvailable(dxrs::sl::Feature::NIS)) throw std::logic_error("NIS is not available");
        for (const auto f : { dxrs::sl::Feature::DLSS, dxrs::sl::Feature::DLSS_G, dxrs::sl::Feature::DLSS_RR })
            if (streamline.IsAvailable(f)) throw std::logic_error("a DLSS feature is reported available");
        dxrs::Raytracing raytracing(device);
        dxrs::Scene scene;
        scene.Load(dxrs::MySceneDesc(0));
        raytracing.SetScene(scene);
        dxrs::CameraController controller;
        controller.SetPosition(scene.Desc.Camera.Position);
        controller.SetLens(1.57079632679489661923f, float(w) / float(h), 1e-2f);
        dxrs::Camera camera;
        controller.Fill(camera, dxrs::Float2{ 0.0f, 0.0f });
        raytracing.SetCamera(camera);
        dxrs::Raytracing::GraphicsSettings gs;
        gs.RenderSize = { w, h }; gs.FrameIndex = 0; gs.Bounces = 8; gs.SamplesPerPixel = 1; gs.IsRussianRouletteEnabled = true;
        raytracing.SetConstants(gs);
        raytracing.UploadConstants();

        auto alloc = [&](uint64_t bytes) { void* p = nullptr; dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &p), ctx, "pt_device_alloc"); return p; };
        void *inColor = alloc(n * 16), *outColor = alloc(n * 16);
        dxrs::ThrowIfFailed(pt_render(ctx, nullptr, inColor, 1, nullptr), ctx, "pt_render");

        // App::ProcessNIS
        dxrs::sl::NISOptions NISOptions;
        NISOptions.mode = dxrs::sl::NISMode::eSharpen;
        NISOptions.sharpness = sharpness;
        NISOptions.hdrMode = static_cast<dxrs::sl::NISHDR>(hdr);
        (void)streamline.SetConstants(NISOptions);
        streamline.Tag(dxrs::sl::BufferType::ScalingInputColor, inColor);
        streamline.Tag(dxrs::sl::BufferType::ScalingOutputColor, outColor);
        if (streamline.Evaluate(dxrs::sl::Feature::NIS, { w, h }) != dxrs::sl::Result::eOk) throw std::runtime_error("Streamline::Evaluate failed");

        std::vector<float> out(n * 8);
        dxrs::ThrowIfFailed(pt_download(ctx, inColor, &out[0], n * 16), ctx, "pt_download");
        dxrs::ThrowIfFailed(pt_download(ctx, outColor, &out[n * 4], n * 16), ctx, "pt_download");
        FILE* f = std::fopen(argv[5], "wb");
        if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) throw std::runtime_error("cannot write output");
        std::fclose(f);

        if (streamline.Evaluate(dxrs::sl::Feature::DLSS, { w, h }) == dxrs::sl::Result::eOk) throw std::logic_error("DLSS was evaluated");
        streamline.Tag(dxrs::sl::BufferType::ScalingOutputColor, nullptr);
        if (streamline.Evaluate(dxrs::sl::Feature::NIS, { w, h }) != dxrs::sl::Result::eErrorMissingInputParameter)
            throw std::logic_error("a missing output tag was not refused");
        std::printf("expected error: missing output tag\n");
        // an in-place call reaches pt_nis_sharpen and is refused there
        streamline.Tag(dxrs::sl::BufferType::ScalingOutputColor, inColor);
        if (streamline.Evaluate(dxrs::sl::Feature::NIS, { w, h }) != dxrs::sl::Result::eErrorInvalidParameter)
            throw std::logic_error("an in-place call was not refused");
        std::printf("expected error: %s\n", pt_last_error(ctx));
        for (void* b : { inColor, outColor }) pt_device_free(ctx, b);
        std::printf("NIS sharpen %ux%u sharpness %g hdr %u\n", w, h, sharpness, hdr);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
