// host_sharc_ex.cpp -- drives pt_render_sharc_ex through the C++ host mirror (Raytracing::Render(radiance, SHARC&, SHARCSettings,
// const DirectLighting*, DenoiserBuffers*)) the way the reference's App::Impl::Render does with ReSTIR-DI, SHARC and DLSS-RR on: a ReBLUR
// frame fills Diffuse / Specular on the device, then two DLSSRayReconstruction frames through the cache read them as their DI.  Writes
// the second frame's radiance (W*H float4) and SpecularHitDistance (W*H float; the buffer is not cleared: only what a frame wrote means
// anything).
// Usage: host_sharc_ex <width> <height> <out.f32>
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
        gs.Denoiser = dxrs::Denoiser::NRDReBLUR;
        raytracing.SetConstants(gs);

        void* bufs[3] = {};
        for (void*& b : bufs) dxrs::ThrowIfFailed(pt_device_alloc(ctx, n * 16, &b), ctx, "pt_device_alloc");
        std::vector<dxrs::Float4> radiance;
        dxrs::Raytracing::DenoiserBuffers db;
        db.Diffuse = bufs[0];
        db.Specular = bufs[1];
        raytracing.Render(radiance, db);

        gs.Denoiser = dxrs::Denoiser::DLSSRayReconstruction;
        raytracing.SetConstants(gs);
        dxrs::SHARC sharc;
        sharc.Configure(1u << 18);
        dxrs::Raytracing::SHARCSettings settings;  // the reference's values
        const dxrs::Raytracing::DirectLighting di{ bufs[0], bufs[1] };
        bool refused = false;
        try { raytracing.Render(radiance, sharc, settings, &di, nullptr); } catch (const std::invalid_argument&) { refused = true; }
        if (!refused) throw std::runtime_error("Render(radiance, sharc, settings, di, nullptr) accepted a denoiser without its buffers");
        if (!sharc.NeedsReset()) throw std::runtime_error("a refused call cleared the restart");
        dxrs::Raytracing::DenoiserBuffers rr;
        rr.SpecularHitDistance = bufs[2];
        std::vector<float> shd(n, 0.0f);
        raytracing.Render(radiance, sharc, settings, &di, &rr);
        if (sharc.NeedsReset()) throw std::runtime_error("the first frame did not clear the restart");
        raytracing.Render(radiance, sharc, settings, &di, &rr);
        dxrs::ThrowIfFailed(pt_download(ctx, bufs[2], shd.data(), n * sizeof(float)), ctx, "pt_download");

        FILE* f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(radiance.data(), sizeof(dxrs::Float4), radiance.size(), f) != radiance.size() || std::fwrite(shd.data(), sizeof(float), n, f) != n)
            throw std::runtime_error("cannot write output");
        std::fclose(f);
        for (void* b : bufs) pt_device_free(ctx, b);
        std::printf("sharc ex: %ux%u\n", w, h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
