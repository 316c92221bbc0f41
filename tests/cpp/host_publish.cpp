// host_publish.cpp -- the frame loop with physics through the C++ host mirror in publishing mode (dxrs::Physics::SetPublishing, row N24):
// the demo scene, Star gravity on, `ticks` rounds of MyScene::TickPhysics -> GBufferGeneration::RenderPublished (MotionVector) ->
// Raytracing::Render, with no download inside the loop; then Physics::Download.  Writes, as float32 words: n, the spheres the physics started
// from (n x 4), the bodies (n x 4 words), the initial linear and angular velocities (n x 3 each), the attractors (4 x 4 words, unused ones
// with Kind = 0xFFFFFFFF), the rotations it started from (n x 4), the spheres and rotations Download put into the scene (n x 4 each), the
// last frame (w x h x 4) and its motion vectors (w x h x 3).
// Usage: host_publish <ticks> <width> <height> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "GBufferGeneration.hpp"
#include "MyScene.hpp"
#include "Physics.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s ticks width height out.bin\n", argv[0]); return 2; }
    try {
        const int ticks = std::atoi(argv[1]);
        const uint32_t w = std::atoi(argv[2]), h = std::atoi(argv[3]);
        dxrs::DeviceContext device;
        PtContext* ctx = device.Get();
        dxrs::MyScene scene(0);
        const std::vector<PtSphere> start = scene.GetSpheres();
        const std::vector<float> startRotations = scene.GetRotations();
        dxrs::Raytracing raytracing(device);
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

        dxrs::Physics physics(device, scene);
        physics.SetPublishing(true);
        scene.SetPhysics(&physics);
        scene.SetStarGravity(true);
        void* motion = nullptr;
        dxrs::ThrowIfFailed(pt_device_alloc(ctx, (uint64_t)w * h * 12, &motion), ctx, "pt_device_alloc");
        dxrs::GBufferGeneration gbuffer;
        gbuffer.GPUBuffers.MotionVector = motion;
        std::vector<dxrs::Float4> radiance;
        for (int k = 0; k < ticks; k++) {
            scene.TickPhysics(0.25);  // a slow frame: the tick is min(1/60, elapsed)
            dxrs::ThrowIfFailed(gbuffer.RenderPublished(ctx), ctx, "pt_render_gbuffer_published");
            raytracing.Render(radiance);
        }
        if (scene.GetSpheres()[0].cy != start[0].cy || std::memcmp(scene.GetSpheres().data(), start.data(), start.size() * sizeof(PtSphere)) != 0)
            throw std::logic_error("publishing mode changed the scene's host copy inside the loop");
        std::vector<float> mv((size_t)w * h * 3);
        dxrs::ThrowIfFailed(pt_download(ctx, motion, mv.data(), mv.size() * sizeof(float)), ctx, "pt_download");
        physics.Download(scene);

        const uint32_t n = scene.GetObjectCount();
        std::vector<float> out;
        auto put = [&](const void* p, size_t words) { const float* f = static_cast<const float*>(p); out.insert(out.end(), f, f + words); };
        out.push_back((float)n);
        put(start.data(), 4 * (size_t)n);
        put(physics.GetBodies().data(), 4 * (size_t)n);
        put(physics.GetInitialLinearVelocities().data(), 3 * (size_t)n);
        put(physics.GetInitialAngularVelocities().data(), 3 * (size_t)n);
        PtPhysicsAttractor att[4];
        std::memset(att, 0xFF, sizeof att);
        for (size_t k = 0; k < physics.GetAttractors().size(); k++) att[k] = physics.GetAttractors()[k];
        put(att, 16);
        put(startRotations.data(), 4 * (size_t)n);
        put(scene.GetSpheres().data(), 4 * (size_t)n);
        put(scene.GetRotations().data(), 4 * (size_t)n);
        put(radiance.data(), 4 * (size_t)w * h);
        put(mv.data(), mv.size());
        FILE* f = std::fopen(argv[4], "wb");
        if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) throw std::runtime_error("cannot write output");
        std::fclose(f);
        dxrs::ThrowIfFailed(pt_device_free(ctx, motion), ctx, "pt_device_free");
        std::printf("published %u bodies, %d ticks\n", n, ticks);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
