// host_nrd_composition.cpp -- drives pt_nrd_composition through the C++ host mirror (PostProcessing::NRDComposition) the way the
// reference's App::Impl::ProcessNRD does: G-buffer and denoiser frame of the demo scene into device buffers, pack, a stand-in for NRD
// (the identity: the packed buffers are bound as the denoised ones), compose.  Also checks that a bad mode is refused.  Writes the
// composed radiance (W*H float4), then the packed Diffuse and Specular (W*H float4 each).
// Usage: host_nrd_composition <width> <height> <Denoiser 2..3> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "NRDComposition.hpp"
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
        raytracing.SetConstants(gs);
        raytracing.UploadConstants();

        auto alloc = [&](uint64_t bytes) { void* p = nullptr; dxrs::ThrowIfFailed(pt_device_alloc(ctx, bytes, &p), ctx, "pt_device_alloc"); return p; };
        void *depth = alloc(n * 4), *da = alloc(n * 12), *sa = alloc(n * 12), *nr = alloc(n * 16);
        void *radiance = alloc(n * 16), *diffuse = alloc(n * 16), *specular = alloc(n * 16);
        dxrs::GBufferGeneration gbuffer;
        gbuffer.GPUBuffers.LinearDepth = depth;
        gbuffer.GPUBuffers.DiffuseAlbedo = da;
        gbuffer.GPUBuffers.SpecularAlbedo = sa;
        gbuffer.GPUBuffers.NormalRoughness = nr;
        dxrs::ThrowIfFailed(gbuffer.Render(ctx), ctx, "GBufferGeneration::Render");
        PtDenoiserOutputs dn{};
        dn.Denoiser = mode;
        dn.Diffuse = diffuse;
        dn.Specular = specular;
        dxrs::ThrowIfFailed(pt_render_denoiser(ctx, nullptr, radiance, 1, &dn, nullptr), ctx, "pt_render_denoiser");

        dxrs::PostProcessing::NRDComposition composition(device);
        composition.Textures = { depth, da, sa, nr, diffuse, specular, diffuse, specular, radiance };
        dxrs::PostProcessing::NRDComposition::Constants constants{ { w, h }, 1, static_cast<dxrs::Denoiser>(mode),
                                                                   dxrs::PostProcessing::NRDComposition::DefaultReBLURHitDistance };
        composition.Process(constants);  // pack
        // ... NRD would denoise here; the identity reads the packed buffers back as the denoised ones
        constants.Pack = 0;
        composition.Process(constants);  // compose
        try {
            constants.Denoiser = dxrs::Denoiser::DLSSRayReconstruction;
            composition.Process(constants);
            throw std::logic_error("DLSSRayReconstruction was accepted");
        } catch (const std::runtime_error& e) {
            std::printf("expected error: %s\n", e.what());
        }

        FILE* f = std::fopen(argv[4], "wb");
        if (!f) throw std::runtime_error("cannot write output");
        for (void* b : { radiance, diffuse, specular }) {
            std::vector<float> c(n * 4);
            dxrs::ThrowIfFailed(pt_download(ctx, b, c.data(), c.size() * 4), ctx, "pt_download");
            if (std::fwrite(c.data(), sizeof(float), c.size(), f) != c.size()) throw std::runtime_error("cannot write output");
        }
        std::fclose(f);
        for (void* b : { depth, da, sa, nr, radiance, diffuse, specular }) pt_device_free(ctx, b);
        std::printf("NRD composition %u: %ux%u\n", mode, w, h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
