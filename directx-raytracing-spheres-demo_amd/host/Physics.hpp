// Physics.hpp -- C++ host mirror of the reference's PhysX wrapper as MyScene drives it (Source/MyScene.ixx:96-110, 228-300, 351-396:
// createRigidDynamic + updateMassAndInertia(density 1), the initial velocities, the forces of Tick and PhysX->Tick) over pt_physics_* (row
// N23, DESIGN.md spec S27), a stand-in for the PhysX SDK, which the reference does not vendor.  No parity with PhysX is claimed.
// The stand-in runs in render space (the layouts of pt_update_spheres / pt_update_rotations: PhysX z negated, Scene::Refresh), so polar
// vectors have z negated and axial vectors x and y.  Tick downloads the poses into the scene; the caller hands them to the renderer
// (pt_update_spheres / Raytracing::UpdateRotations).  In publishing mode (SetPublishing, row N24, spec S28) Tick hands them to the frames
// on the device instead (pt_physics_publish): no download and no wait inside the frame loop; Download(scene) brings the poses into the
// scene for callers that want them on the host.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "MyScene.hpp"
#include "Raytracing.hpp"

namespace dxrs {

class Physics : public PhysicsBackend {
public:
    static constexpr float kTwoPi = 6.28318530717958647692f;
    float LargeRadiusFactor = 4.0f;  // bodies above this many median radii are flagged PT_PHYSICS_LARGE

    Physics(DeviceContext& deviceContext, MyScene& scene, const PtPhysicsSettings* settings = nullptr) : m_ctx(deviceContext.Get())
    {
        if (!m_ctx) throw std::invalid_argument("null device context");
        const auto& objects = scene.Desc.RenderObjects;
        const auto& spheres = scene.GetSpheres();
        const size_t n = objects.size();
        m_bodies.assign(n, PtPhysicsBody{});
        m_linearVelocities.assign(3 * n, 0.0f);
        m_angularVelocities.assign(3 * n, 0.0f);
        std::vector<float> radii(n);
        for (size_t i = 0; i < n; i++) radii[i] = objects[i].Radius;
        std::nth_element(radii.begin(), radii.begin() + n / 2, radii.end());
        const float median = n ? radii[n / 2] : 0.0f;
        constexpr float A = 0.5f, omega = kTwoPi / Spring::Period;
        for (size_t i = 0; i < n; i++) {
            const auto& o = objects[i];
            PtPhysicsBody& b = m_bodies[i];
            b.InvMass = 1.0f / (4.0f / 3.0f * 3.14159265358979323846f * o.Radius * o.Radius * o.Radius);  // updateMassAndInertia(rigidDynamic, 1)
            if (o.Radius > LargeRadiusFactor * median) b.Flags |= PT_PHYSICS_LARGE;
            if (o.Name == ObjectNames::HarmonicOscillator) {
                b.Flags |= PT_PHYSICS_SPRING;
                b.SpringY0 = Spring::PositionY;
                b.SpringOmega2 = omega * omega;  // k / m = 4 pi^2 / T^2 (SimpleHarmonicMotion::Spring::CalculateConstant)
                m_linearVelocities[3 * i + 1] = -A * omega * std::sin(0.0f - o.Position.x);  // CalculateVelocity(A, omega, 0, x), MyScene.ixx:228
            } else if (o.Name == ObjectNames::Moon) {
                m_moon = static_cast<int>(i);
            } else if (o.Name == ObjectNames::Earth) {
                m_earth = static_cast<int>(i);
                m_angularVelocities[3 * i + 1] = -(kTwoPi / 15.0f);  // RotationPeriod = 15 (MyScene.ixx:290); axial: y negated in render space
            } else if (o.Name == ObjectNames::Star) {
                m_star = static_cast<int>(i);
                b.InvMass = 0.0f;  // setMass(0)
            }
        }
        if (m_moon >= 0 && m_earth >= 0) {
            // UniversalGravitation::CalculateMass(r, T) = 4 pi^2 r^3 / (G T^2): only G m enters the pull; the Earth itself is as good as immovable
            const auto &e = objects[m_earth].Position, &m = objects[m_moon].Position;
            const float dx = e.x - m.x, dy = e.y - m.y, dz = e.z - m.z;
            const float r = std::sqrt(dx * dx + dy * dy + dz * dz), T = 10.0f;  // OrbitalPeriod
            m_earthGM = 4.0f * 3.14159265358979323846f * 3.14159265358979323846f * r * r * r / (T * T);
            m_bodies[m_earth].InvMass = 6.6743e-11f / m_earthGM;
            const float speed = std::sqrt(m_earthGM / r);  // CalculateFirstCosmicSpeed
            // PhysX space: speed * (-n.z, 0, n.x), n = (earth - moon) / r; render space negates z (MyScene.ixx:283)
            m_linearVelocities[3 * m_moon] = speed * -(dz / r);
            m_linearVelocities[3 * m_moon + 2] = -(speed * (dx / r));
            m_angularVelocities[3 * m_moon + 1] = -(speed / r);  // tidally locked
        }
        ThrowIfFailed(pt_physics_create(m_ctx, spheres.data(), m_bodies.data(), m_linearVelocities.data(), m_angularVelocities.data(), scene.GetRotations().data(),
                                        static_cast<uint32_t>(n), settings), m_ctx, "pt_physics_create");
        SetAttractors(scene);
    }

    ~Physics() override { pt_physics_destroy(m_ctx); }
    Physics(const Physics&) = delete;
    Physics& operator=(const Physics&) = delete;

    // publishing: Tick publishes the poses on the device (the context needs the scene the physics was made from) and leaves the scene's
    // host copy and GetReport() as they are
    void SetPublishing(bool publishing) { m_publishing = publishing; }
    bool IsPublishing() const { return m_publishing; }

    // PhysX->Tick after the forces of MyScene::Tick: one step, then the poses back into the scene -- or, publishing, on to the frames
    void Tick(MyScene& scene, float elapsedSeconds) override
    {
        SetAttractors(scene);
        if (m_publishing) {
            ThrowIfFailed(pt_physics_step(m_ctx, elapsedSeconds, 1, nullptr), m_ctx, "pt_physics_step");
            ThrowIfFailed(pt_physics_publish(m_ctx), m_ctx, "pt_physics_publish");
            return;
        }
        ThrowIfFailed(pt_physics_step(m_ctx, elapsedSeconds, 1, &m_report), m_ctx, "pt_physics_step");
        Download(scene);
    }

    // the simulation's current poses into the scene (waits for the context's stream)
    void Download(MyScene& scene)
    {
        auto& objects = scene.Desc.RenderObjects;
        m_spheres.resize(objects.size());
        m_rotations.resize(4 * objects.size());
        ThrowIfFailed(pt_physics_download(m_ctx, m_spheres.data(), m_rotations.data(), nullptr, nullptr), m_ctx, "pt_physics_download");
        for (size_t i = 0; i < objects.size(); i++) {
            objects[i].Position = { m_spheres[i].cx, m_spheres[i].cy, -m_spheres[i].cz };
            objects[i].Rotation.x = -m_rotations[4 * i]; objects[i].Rotation.y = -m_rotations[4 * i + 1];
            objects[i].Rotation.z = m_rotations[4 * i + 2]; objects[i].Rotation.w = m_rotations[4 * i + 3];
        }
        scene.Refresh();
    }

    const PtPhysicsReport& GetReport() const { return m_report; }
    const std::vector<PtPhysicsBody>& GetBodies() const { return m_bodies; }
    const std::vector<float>& GetInitialLinearVelocities() const { return m_linearVelocities; }
    const std::vector<float>& GetInitialAngularVelocities() const { return m_angularVelocities; }
    const std::vector<PtPhysicsAttractor>& GetAttractors() const { return m_attractors; }

private:
    // MyScene.ixx:378-392: the Earth pulls the Moon always and every body once G is pressed; the Star pulls every body once H is pressed
    void SetAttractors(const MyScene& scene)
    {
        std::vector<PtPhysicsAttractor> a;
        if (m_earth >= 0 && (scene.IsEarthGravityEnabled() || m_moon >= 0))
            a.push_back({ static_cast<uint32_t>(m_earth), PT_PHYSICS_INVERSE_SQUARE, m_earthGM, scene.IsEarthGravityEnabled() ? PT_PHYSICS_ALL_BODIES : static_cast<uint32_t>(m_moon) });
        if (m_star >= 0 && scene.IsStarGravityEnabled()) a.push_back({ static_cast<uint32_t>(m_star), PT_PHYSICS_CONSTANT, 10.0f, PT_PHYSICS_ALL_BODIES });
        const bool same = a.size() == m_attractors.size() && std::equal(a.begin(), a.end(), m_attractors.begin(), [](const PtPhysicsAttractor& x, const PtPhysicsAttractor& y) {
            return x.Body == y.Body && x.Kind == y.Kind && x.Strength == y.Strength && x.Target == y.Target; });
        if (same && m_attractorsSet) return;
        ThrowIfFailed(pt_physics_set_attractors(m_ctx, a.data(), static_cast<uint32_t>(a.size())), m_ctx, "pt_physics_set_attractors");
        m_attractors = a;
        m_attractorsSet = true;
    }

    PtContext* m_ctx;
    int m_moon = -1, m_earth = -1, m_star = -1;
    float m_earthGM = 0.0f;
    bool m_attractorsSet = false, m_publishing = false;
    std::vector<PtPhysicsBody> m_bodies;
    std::vector<float> m_linearVelocities, m_angularVelocities, m_rotations;
    std::vector<PtSphere> m_spheres;
    std::vector<PtPhysicsAttractor> m_attractors;
    PtPhysicsReport m_report{};
};

}  // namespace dxrs
