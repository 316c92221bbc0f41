// host_sharc_ff.cpp -- drives the radiance cache's anti-firefly filter (row N19) through the C++ host mirror the way the reference's
// App::Impl::Render fills its settings (App.cpp:1270-1278: DownscaleFactor, RoughnessThreshold, IsHashGridVisualizationEnabled, then
// SceneScale and IsAntiFireflyEnabled = true): four frames of Raytracing::Render(radiance, SHARC&, SHARCSettings) without DI; then, the
// cache restarted, a ReBLUR frame fills Diffuse / Specular on the device and two DLSSRayReconstruction frames read them as their DI
// through the five-argument form.  Writes the fourth plain frame's radiance and the last frame's (W*H float4 each).
// Usage: host_sharc_ff <width> <height> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "MyScene.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s width height out.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]);
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
        dxrs::Camera camera;
        controller.Fill(camera, dxrs::Float2{});
        raytracing.SetCamera(camera);
        dxrs::Raytracing::GraphicsSettings gs;
        gs.RenderSize = { w, h }; gs.Bounces = 8; gs.SamplesPerPixel = 1; gs.IsRussianRouletteEnabled = true;

        dxrs::SHARC sharc;
        sharc.Configure(1u << 14);
        dxrs::Raytracing::SHARCSettings settings;
        settings.DownscaleFactor = 4;
        settings.RoughnessThreshold = 0.4f;
        settings.IsHashGridVisualizationEnabled = 0;
        settings.SceneScale = 5.0f;  // (large voxels: at this frame size a voxel gathers the history the filter needs)
        settings.IsAntiFireflyEnabled = true;
        std::vector<dxrs::Float4> plain, radiance;
        for (uint32_t f = 0; f < 4; f++) {
            gs.FrameIndex = f;
            raytracing.SetConstants(gs);
            raytracing.Render(plain, sharc, settings);
            if (sharc.NeedsReset()) throw std::runtime_error("a frame did not clear the restart");
        }

        void* bufs[3] = {};
        for (void*& b : bufs) dxrs::ThrowIfFailed(pt_device_alloc(ctx, n * 16, &b), ctx, "pt_device_alloc");
        gs.FrameIndex = 0;
        gs.Denoiser = dxrs::Denoiser::NRDReBLUR;
        raytracing.SetConstants(gs);
        dxrs::Raytracing::DenoiserBuffers db;
        db.Diffuse = bufs[0];
        db.Specular = bufs[1];
        raytracing.Render(radiance, db);

        gs.Denoiser = dxrs::Denoiser::DLSSRayReconstruction;
        raytracing.SetConstants(gs);
        bool refused = false;
        try { raytracing.Render(radiance, sharc, settings); } catch (const std::invalid_argument&) { refused = true; }
        if (!refused) throw std::runtime_error("Render(radiance, sharc, settings) with the filter accepted a denoiser without its buffers");
        sharc.Configure(1u << 14);
        const dxrs::Raytracing::DirectLighting di{ bufs[0], bufs[1] };
        dxrs::Raytracing::DenoiserBuffers rr;
        rr.SpecularHitDistance = bufs[2];
        raytracing.Render(radiance, sharc, settings, &di, &rr);
        raytracing.Render(radiance, sharc, settings, &di, &rr);

        FILE* f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(plain.data(), sizeof(dxrs::Float4), plain.size(), f) != plain.size() ||
            std::fwrite(radiance.data(), sizeof(dxrs::Float4), radiance.size(), f) != radiance.size())
            throw std::runtime_error("cannot write output");
        std::fclose(f);
        for (void* b : bufs) pt_device_free(ctx, b);
        std::printf("sharc ff: %ux%u\n", w, h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
