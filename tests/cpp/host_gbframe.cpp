// host_gbframe.cpp -- drives row N27 through the C++ host mirror the way the reference's App::Impl::Render orders it: the G-buffer pass
// (GBufferGeneration::Render, into float32 buffers and into textures of the reference's formats), then the frame whose primary surface is
// that G-buffer (Raytracing::Render(radiance, GBufferTextures)), queued right behind it.  Writes three W*H float4 frames -- from the float32
// G-buffer, from the packed one, and Render's own -- and then the packed channels BaseColorMetalness (4 B), NormalRoughness (8 B), IOR (2 B)
// and Radiance (8 B) as downloaded, then the PtCamera the frames used (sizeof(PtCamera) bytes).
// Usage: host_gbframe <width> <height> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s width height out.bin\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]);
        const uint64_t px = (uint64_t)w * h;
        const uint32_t f32_bytes[13] = { 16, 8, 8, 4, 4, 12, 16, 12, 12, 16, 4, 4, 12 };
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
        controller.FillMatrices(camera);
        raytracing.SetCamera(camera);
        dxrs::Raytracing::GraphicsSettings gs;
        gs.RenderSize = { w, h }; gs.FrameIndex = 4; gs.Bounces = 6; gs.SamplesPerPixel = 2; gs.IsRussianRouletteEnabled = true;
        raytracing.SetConstants(gs);
        raytracing.UploadConstants();

        void *f32[13] = {}, *packed[13] = {};
        for (int k = 0; k < 13; k++) {
            dxrs::ThrowIfFailed(pt_device_alloc(ctx, px * f32_bytes[k], &f32[k]), ctx, "pt_device_alloc");
            dxrs::ThrowIfFailed(pt_device_alloc(ctx, px * dxrs::GBufferGeneration::PackedTexelBytes[k], &packed[k]), ctx, "pt_device_alloc");
        }
        const auto bind = [](dxrs::GBufferGeneration::Textures& t, void* const* b) {
            void** slots[13] = { &t.Position, &t.FlatNormal, &t.GeometricNormal, &t.LinearDepth, &t.NormalizedDepth, &t.MotionVector, &t.BaseColorMetalness,
                                 &t.DiffuseAlbedo, &t.SpecularAlbedo, &t.NormalRoughness, &t.IOR, &t.Transmission, &t.Radiance };
            for (int k = 0; k < 13; k++) *slots[k] = b[k];
        };
        const auto textures_of = [](void* const* b, bool is_packed) {
            dxrs::Raytracing::GBufferTextures t;
            t.Packed = is_packed;
            t.Position = b[0]; t.FlatNormal = b[1]; t.GeometricNormal = b[2]; t.BaseColorMetalness = b[6]; t.NormalRoughness = b[9]; t.IOR = b[10];
            t.Transmission = b[11]; t.Radiance = b[12];
            return t;
        };
        dxrs::GBufferGeneration gbuffer;
        bind(gbuffer.GPUBuffers, f32);
        std::vector<dxrs::Float4> from_f32, from_packed, plain;
        dxrs::ThrowIfFailed(gbuffer.Render(ctx), ctx, "GBufferGeneration::Render");
        raytracing.Render(from_f32, textures_of(f32, false));  // (queued behind the pass on the same lane: no wait in between)
        dxrs::GBufferGeneration::PackedTextures pt;
        bind(pt, packed);
        dxrs::ThrowIfFailed(gbuffer.Render(ctx, pt), ctx, "GBufferGeneration::Render (packed)");
        raytracing.Render(from_packed, textures_of(packed, true));
        raytracing.Render(plain);

        FILE* f = std::fopen(argv[3], "wb");
        bool ok = f != nullptr;
        for (const auto* img : { &from_f32, &from_packed, &plain }) ok = ok && std::fwrite(img->data(), sizeof(dxrs::Float4), img->size(), f) == img->size();
        for (int k : { 6, 9, 10, 12 }) {
            std::vector<unsigned char> c(px * dxrs::GBufferGeneration::PackedTexelBytes[k]);
            dxrs::ThrowIfFailed(pt_download(ctx, packed[k], c.data(), c.size()), ctx, "pt_download");
            ok = ok && std::fwrite(c.data(), 1, c.size(), f) == c.size();
        }
        const PtCamera used = dxrs::ToPt(camera);
        ok = ok && std::fwrite(&used, sizeof used, 1, f) == 1;
        if (!ok) throw std::logic_error("cannot write output");
        std::fclose(f);
        for (int k = 0; k < 13; k++) { pt_device_free(ctx, f32[k]); pt_device_free(ctx, packed[k]); }
        std::printf("gbframe %ux%u\n", w, h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
