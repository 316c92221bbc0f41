// host_lens.cpp -- drives pt_render_lens through the C++ host mirror (Raytracing::RenderThinLens): the demo scene, the controller's
// SetFocusDistance, Camera::ApertureRadius written by the caller (the reference's controller has no setter).  Writes the lens frame
// (W*H float4), the same camera's frame with ApertureRadius = 0 (W*H float4), Render's frame (W*H float4) and the PtCamera the lens frame
// used (sizeof(PtCamera) bytes).
// Usage: host_lens <width> <height> <aperture> <focus distance> <out.f32>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "MyScene.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 6) { std::fprintf(stderr, "usage: %s width height aperture focus_distance out.f32\n", argv[0]); return 2; }
    try {
        const uint32_t w = std::atoi(argv[1]), h = std::atoi(argv[2]);
        dxrs::DeviceContext device;
        dxrs::Raytracing raytracing(device);
        dxrs::Scene scene;
        scene.Load(dxrs::MySceneDesc(0));
        raytracing.SetScene(scene);
        dxrs::CameraController controller;
        controller.SetPosition(scene.Desc.Camera.Position);
        controller.SetLens(1.57079632679489661923f, float(w) / float(h));
        controller.SetFocusDistance(static_cast<float>(std::atof(argv[4])));
        dxrs::Camera camera;
        controller.Fill(camera, dxrs::Float2{});
        camera.ApertureRadius = static_cast<float>(std::atof(argv[3]));
        raytracing.SetCamera(camera);
        dxrs::Raytracing::GraphicsSettings gs;
        gs.RenderSize = { w, h }; gs.FrameIndex = 2; gs.Bounces = 6; gs.SamplesPerPixel = 2; gs.IsRussianRouletteEnabled = true;
        raytracing.SetConstants(gs);
        std::vector<dxrs::Float4> lens, pinhole, plain;
        raytracing.RenderThinLens(lens);
        const PtCamera used = dxrs::ToPt(camera);
        camera.ApertureRadius = 0.0f;
        raytracing.SetCamera(camera);
        raytracing.RenderThinLens(pinhole);
        raytracing.Render(plain);

        bool refused = false;
        camera.ApertureRadius = -1.0f;
        raytracing.SetCamera(camera);  // (pt_set_camera accepts anything)
        try { raytracing.RenderThinLens(plain); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) throw std::logic_error("RenderThinLens accepted a negative ApertureRadius");

        FILE* f = std::fopen(argv[5], "wb");
        bool ok = f != nullptr;
        for (const auto* img : { &lens, &pinhole, &plain }) ok = ok && std::fwrite(img->data(), sizeof(dxrs::Float4), img->size(), f) == img->size();
        ok = ok && std::fwrite(&used, sizeof used, 1, f) == 1;
        if (!ok) throw std::logic_error("cannot write output");
        std::fclose(f);
        std::printf("lens: %ux%u\n", w, h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
