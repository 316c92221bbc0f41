// host_physics.cpp -- drives pt_physics_* through the C++ host mirror (dxrs::Physics, MyScene::TickPhysics) the way the reference's
// MyScene::Tick does with the H key pressed: the demo scene, Star gravity on, `ticks` ticks of 1/60 s.  Writes, as float32 words: n, the
// spheres the physics started from (n x 4), the bodies (n x 4 words), the initial linear and angular velocities (n x 3 each), the attractors
// (4 x 4 words, unused ones with Kind = 0xFFFFFFFF), the rotations it started from (n x 4), then the spheres and rotations after the last tick (n x 4 each) as the scene holds them.
// Usage: host_physics <ticks> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MyScene.hpp"
#include "Physics.hpp"
#include "Raytracing.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s ticks out.bin\n", argv[0]); return 2; }
    try {
        const int ticks = std::atoi(argv[1]);
        dxrs::DeviceContext device;
        dxrs::MyScene scene(0);
        const std::vector<PtSphere> start = scene.GetSpheres();
        const std::vector<float> startRotations = scene.GetRotations();
        dxrs::Physics physics(device, scene);
        scene.SetPhysics(&physics);
        scene.SetStarGravity(true);
        uint32_t contacts = 0;
        for (int k = 0; k < ticks; k++) {
            scene.TickPhysics(0.25);  // a slow frame: the tick is min(1/60, elapsed)
            contacts += physics.GetReport().Contacts;
        }
        if (physics.GetReport().Steps != (uint32_t)ticks) throw std::logic_error("the report's step count is not the number of ticks");
        if (std::fabs(scene.GetTime() - ticks / 60.0) > 1e-9) throw std::logic_error("the scene's time did not advance by 1/60 per tick");
        scene.SetRunning(false);
        scene.TickPhysics(0.25);
        if (physics.GetReport().Steps != (uint32_t)ticks) throw std::logic_error("a static scene was ticked");

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
        FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) throw std::runtime_error("cannot write output");
        std::fclose(f);
        std::printf("physics %u bodies, %d ticks, %u contacts\n", n, ticks, contacts);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
