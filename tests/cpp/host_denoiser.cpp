// host_denoiser.cpp -- drives pt_render_denoiser through the C++ host mirror (Raytracing::Render(radiance, DenoiserBuffers&)) the way
// the reference's App::Impl::Render does with a denoiser selected.  Also checks that
// Render(radiance) still refuses a denoiser.  Writes out (W*H float4), then the mode's buffers (Diffuse, Specular float4 or
// SpecularHitDistance float).
// Usage: host_denoiser <width> <height> <Denoiser 1..3> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "MyScene.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s width height denoiser out.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]), mode = std::atoi(argv[3]);
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
        gs.Denoiser = static_cast<dxrs::Denoiser>(mode);
        raytracing.SetConstants(gs);
        std::vector<dxrs::Float4> radiance;
        bool refused = false;
        try { raytracing.Render(radiance); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) throw std::runtime_error("Render(radiance) accepted a denoiser");

        const uint64_t texel = mode == 1 ? 4 : 16;
        std::vector<void*> bufs(mode == 1 ? 1 : 2, nullptr);
        for (void*& b : bufs) dxrs::ThrowIfFailed(pt_device_alloc(ctx, n * texel, &b), ctx, "pt_device_alloc");  // (texels a mode leaves alone are not compared)
        dxrs::Raytracing::DenoiserBuffers db;
        if (mode == 1) db.SpecularHitDistance = bufs[0];
        else { db.Diffuse = bufs[0]; db.Specular = bufs[1]; }
        raytracing.Render(radiance, db);

        FILE* f = std::fopen(argv[4], "wb");
        if (!f || std::fwrite(radiance.data(), sizeof(dxrs::Float4), radiance.size(), f) != radiance.size()) throw std::runtime_error("cannot write output");
        for (void* b : bufs) {
            std::vector<float> c(n * texel / 4);
            dxrs::ThrowIfFailed(pt_download(ctx, b, c.data(), c.size() * 4), ctx, "pt_download");
            if (std::fwrite(c.data(), sizeof(float), c.size(), f) != c.size()) throw std::runtime_error("cannot write output");
            pt_device_free(ctx, b);
        }
        std::fclose(f);
        std::printf("denoiser %u: %ux%u\n", mode, w, h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
