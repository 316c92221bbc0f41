// host_nrd_reblur.cpp -- drives pt_nrd_reblur through the C++ host mirror (dxrs::NRD with UseReblurStandIn) the way the reference's
// App::Impl::ProcessNRD does in its ReBLUR branch, for a few frames of a resting camera: G-buffer and denoiser frame of the demo scene
// into device buffers, pack, NRD::NewFrame / Tag / SetConstants / Denoise, compose.  The first frame is CLEAR_AND_RESTART.  Also checks
// that the opt-in is off by default and that bad ReblurSettings are refused.  Writes the composed radiance of every frame (frames * W*H
// float4).
// Usage: host_nrd_reblur <width> <height> <frames> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "NRD.hpp"
#include "NRDComposition.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s width height frames out.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]), frames = std::atoi(argv[3]), mode = 2;
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
        void *depth = alloc(n * 4), *mv = alloc(n * 12), *da = alloc(n * 12), *sa = alloc(n * 12), *nr = alloc(n * 16);
        void *radiance = alloc(n * 16), *diffuse = alloc(n * 16), *specular = alloc(n * 16), *denoisedDiffuse = alloc(n * 16),
             *denoisedSpecular = alloc(n * 16);
        dxrs::GBufferGeneration gbuffer;
        gbuffer.GPUBuffers.LinearDepth = depth;
        gbuffer.GPUBuffers.MotionVector = mv;
        gbuffer.GPUBuffers.DiffuseAlbedo = da;
        gbuffer.GPUBuffers.SpecularAlbedo = sa;
        gbuffer.GPUBuffers.NormalRoughness = nr;
        dxrs::PostProcessing::NRDComposition composition(device);
        composition.Textures = { depth, da, sa, nr, diffuse, specular, denoisedDiffuse, denoisedSpecular, radiance };
        dxrs::NRD nrd(device);
        if (nrd.IsReblurStandInUsed()) throw std::logic_error("the ReBLUR stand-in is on by default");
        nrd.UseReblurStandIn(true);
        const dxrs::nrd::Identifier ids[] = { dxrs::nrd::Identifier::REBLUR };
        FILE* f = std::fopen(argv[4], "wb");
        if (!f) throw std::runtime_error("cannot write output");
        for (uint32_t frame = 0; frame < frames; frame++) {
            dxrs::Camera camera;
            controller.Fill(camera, dxrs::Float2{});
            raytracing.SetCamera(camera);
            dxrs::Raytracing::GraphicsSettings gs;
            gs.RenderSize = { w, h }; gs.FrameIndex = frame; gs.Bounces = 8; gs.SamplesPerPixel = 1; gs.IsRussianRouletteEnabled = true;
            raytracing.SetConstants(gs);
            raytracing.UploadConstants();
            dxrs::ThrowIfFailed(gbuffer.Render(ctx), ctx, "GBufferGeneration::Render");
            PtDenoiserOutputs dn{};
            dn.Denoiser = mode;
            dn.Diffuse = diffuse;
            dn.Specular = specular;
            dxrs::ThrowIfFailed(pt_render_denoiser(ctx, nullptr, radiance, 1, &dn, nullptr), ctx, "pt_render_denoiser");
            dxrs::PostProcessing::NRDComposition::Constants constants{ { w, h }, 1, static_cast<dxrs::Denoiser>(mode),
                                                                       dxrs::PostProcessing::NRDComposition::DefaultReBLURHitDistance };
            composition.Process(constants);  // pack

            nrd.NewFrame();
            using dxrs::nrd::ResourceType;
            nrd.Tag(ResourceType::IN_VIEWZ, depth);
            nrd.Tag(ResourceType::IN_MV, mv);
            nrd.Tag(ResourceType::IN_BASECOLOR_METALNESS, nullptr);
            nrd.Tag(ResourceType::IN_NORMAL_ROUGHNESS, nr);
            nrd.Tag(ResourceType::IN_DIFF_RADIANCE_HITDIST, diffuse);
            nrd.Tag(ResourceType::IN_SPEC_RADIANCE_HITDIST, specular);
            nrd.Tag(ResourceType::OUT_DIFF_RADIANCE_HITDIST, denoisedDiffuse);
            nrd.Tag(ResourceType::OUT_SPEC_RADIANCE_HITDIST, denoisedSpecular);
            dxrs::nrd::CommonSettings common{};
            common.rectSize[0] = static_cast<uint16_t>(w);
            common.rectSize[1] = static_cast<uint16_t>(h);
            common.frameIndex = frame;
            common.accumulationMode = frame == 0 ? dxrs::nrd::AccumulationMode::CLEAR_AND_RESTART : dxrs::nrd::AccumulationMode::CONTINUE;
            common.isBaseColorMetalnessAvailable = false;
            nrd.SetConstants(common);
            nrd.SetConstants(dxrs::nrd::Identifier::REBLUR, dxrs::nrd::ReblurSettings{});
            nrd.Denoise(ids);

            constants.Pack = 0;
            composition.Process(constants);  // compose
            std::vector<float> c(n * 4);
            dxrs::ThrowIfFailed(pt_download(ctx, radiance, c.data(), c.size() * 4), ctx, "pt_download");
            if (std::fwrite(c.data(), sizeof(float), c.size(), f) != c.size()) throw std::runtime_error("cannot write output");
        }
        std::fclose(f);
        try {
            dxrs::nrd::ReblurSettings bad{};
            bad.maxBlurRadius = 65.0f;
            nrd.SetConstants(dxrs::nrd::Identifier::REBLUR, bad);
            nrd.Denoise(ids);
            throw std::logic_error("a MaxBlurRadius of 65 was accepted");
        } catch (const std::runtime_error& e) {
            std::printf("expected error: %s\n", e.what());
        }
        for (void* b : { depth, mv, da, sa, nr, radiance, diffuse, specular, denoisedDiffuse, denoisedSpecular }) pt_device_free(ctx, b);
        std::printf("NRD ReBLUR stand-in: %ux%u, %u frames\n", w, h, frames);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
