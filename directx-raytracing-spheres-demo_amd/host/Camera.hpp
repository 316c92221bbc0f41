// Camera.hpp -- host mirror of Source/Camera.ixx: the `Camera` constant-buffer struct (:16-36, same
// field names and byte layout as PtCamera) and `CameraController` (:38-177).  The bounce loop reads only
// Position / Right / Up / Forward (lens-scaled, un-normalised), NearDepth, FarDepth and Jitter
// (Shaders/Camera.hlsli:27-41).  Fill leaves the eight matrices as they are; FillMatrices adds them (App.cpp:531-553)
// for the G-buffer pass (pt_render_gbuffer: depths and motion vectors, DESIGN.md spec S12).
#pragma once

#include <cmath>
#include <cstring>
#include <limits>
#include <utility>

#include "Material.hpp"

namespace dxrs {

struct alignas(256) Camera {  // Camera.ixx:16-36 (D3D12_CONSTANT_BUFFER_DATA_PLACEMENT_ALIGNMENT = 256)
    uint32_t IsNormalizedDepthReversed{};
    Float3 PreviousPosition, Position;
    float _{};
    Float3 RightDirection;
    float _1{};
    Float3 UpDirection;
    float _2{};
    Float3 ForwardDirection;
    float ApertureRadius{}, NearDepth{}, FarDepth{};
    Float2 Jitter;
    float Matrices[8][16]{};
};
static_assert(sizeof(Camera) == 768, "alignas(256) payload of 608 B");

inline PtCamera ToPt(const Camera& c)
{
    PtCamera r;
    std::memcpy(&r, &c, sizeof r);
    return r;
}

inline Float3 operator+(Float3 a, Float3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline Float3 operator-(Float3 a, Float3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline Float3 operator*(Float3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }
inline Float3 operator/(Float3 a, float s) { return { a.x / s, a.y / s, a.z / s }; }

namespace detail {
inline float Length(Float3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
inline Float3 Cross(Float3 a, Float3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
inline Float3 Normalized(Float3 a) { return a / Length(a); }
}  // namespace detail

struct Quaternion {
    float x{}, y{}, z{}, w = 1;

    static Quaternion CreateFromAxisAngle(Float3 axis, float angle)
    {
        const auto n = detail::Normalized(axis);
        const float s = std::sin(angle * 0.5f);
        return { n.x * s, n.y * s, n.z * s, std::cos(angle * 0.5f) };
    }
    static Quaternion CreateFromYawPitchRoll(float yaw, float pitch, float roll)
    {
        const float cy = std::cos(yaw * 0.5f), sy = std::sin(yaw * 0.5f);
        const float cp = std::cos(pitch * 0.5f), sp = std::sin(pitch * 0.5f);
        const float cr = std::cos(roll * 0.5f), sr = std::sin(roll * 0.5f);
        return { cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr, cy * cp * sr - sy * sp * cr, cy * cp * cr + sy * sp * sr };
    }
    Quaternion Normalized() const
    {
        const float l = std::sqrt(x * x + y * y + z * z + w * w);
        return { x / l, y / l, z / l, w / l };
    }
    // SimpleMath semantics: (a * b) applies a first, then b.
    friend Quaternion operator*(const Quaternion& a, const Quaternion& b)
    {
        return { b.w * a.x + b.x * a.w + b.y * a.z - b.z * a.y,
                 b.w * a.y - b.x * a.z + b.y * a.w + b.z * a.x,
                 b.w * a.z + b.x * a.y - b.y * a.x + b.z * a.w,
                 b.w * a.w - b.x * a.x - b.y * a.y - b.z * a.z };
    }
    Float3 Rotate(Float3 v) const
    {
        using namespace detail;
        const Float3 u{ x, y, z };
        const Float3 t = Cross(u, v) * 2.0f;
        return v + t * w + Cross(u, t);
    }
};

struct CameraController {  // Camera.ixx:38-177
    explicit CameraController(bool isNormalizedDepthReversed = true) : m_isNormalizedDepthReversed(isNormalizedDepthReversed) {}

    const Float3& GetPosition() const { return m_position; }
    void SetPosition(const Float3& value) { m_position = value; }

    const Float3& GetRightDirection() const { return m_rightDirection; }
    const Float3& GetUpDirection() const { return m_upDirection; }
    const Float3& GetForwardDirection() const { return m_forwardDirection; }

    Float3 GetNormalizedRightDirection() const { return detail::Normalized(m_rightDirection); }
    Float3 GetNormalizedUpDirection() const { return detail::Normalized(m_upDirection); }
    Float3 GetNormalizedForwardDirection() const { return detail::Normalized(m_forwardDirection); }

    void SetDirections(const Float3& forwardDirection, const Float3& upDirection = { 0, 1, 0 }, bool setFocusDistance = true)
    {
        using namespace detail;
        m_forwardDirection = forwardDirection;
        m_rightDirection = Cross(upDirection, forwardDirection);
        m_upDirection = Cross(m_forwardDirection, m_rightDirection);
        if (setFocusDistance) {
            SetFocusDistance(Length(m_forwardDirection));
        } else {
            m_rightDirection = GetNormalizedRightDirection() * m_rightDirectionLength;
            m_upDirection = GetNormalizedUpDirection() * m_upDirectionLength;
            m_forwardDirection = GetNormalizedForwardDirection() * m_forwardDirectionLength;
        }
    }

    const Quaternion& GetRotation() const { return m_rotation; }

    void SetRotation(const Quaternion& value)
    {
        using namespace detail;
        m_rotation = value.Normalized();
        m_forwardDirection = Normalized(m_rotation.Rotate({ 0, 0, 1 }));
        m_rightDirection = Normalized(m_rotation.Rotate({ 1, 0, 0 }));
        m_upDirection = Cross(m_forwardDirection, m_rightDirection) * m_upDirectionLength;
        m_forwardDirection = m_forwardDirection * m_forwardDirectionLength;
        m_rightDirection = m_rightDirection * m_rightDirectionLength;
    }

    void LookAt(const Float3& position, const Float3& upDirection = { 0, 1, 0 }, bool setFocusDistance = true)
    {
        using namespace detail;
        SetDirections(position - m_position, upDirection, setFocusDistance);
    }

    float GetFocusDistance() const { return m_forwardDirectionLength; }

    void SetFocusDistance(float value)
    {
        m_rightDirectionLength *= value / m_forwardDirectionLength;
        m_upDirectionLength *= value / m_forwardDirectionLength;
        m_forwardDirectionLength = value;
        m_rightDirection = GetNormalizedRightDirection() * m_rightDirectionLength;
        m_upDirection = GetNormalizedUpDirection() * m_upDirectionLength;
        m_forwardDirection = GetNormalizedForwardDirection() * m_forwardDirectionLength;
    }

    void Translate(const Float3& value) { using namespace detail; SetPosition(m_position + value); }

    void Rotate(float yaw, float pitch, float roll = 0)
    {
        SetRotation(m_rotation * Quaternion::CreateFromAxisAngle(m_rightDirection, -pitch) * Quaternion::CreateFromAxisAngle({ 0, 1, 0 }, yaw)
                    * Quaternion::CreateFromAxisAngle(m_forwardDirection, -roll));
    }

    float GetHorizontalFieldOfView() const { return m_horizontalFieldOfView; }
    float GetVerticalFieldOfView() const { return 2 * std::atan(std::tan(m_horizontalFieldOfView / 2) * m_aspectRatio); }
    float GetAspectRatio() const { return m_aspectRatio; }
    float GetNearDepth() const { return m_nearDepth; }
    float GetFarDepth() const { return m_farDepth; }

    void SetLens(float horizontalFieldOfView, float aspectRatio)
    {
        using namespace detail;
        m_horizontalFieldOfView = horizontalFieldOfView;
        m_aspectRatio = aspectRatio;
        m_rightDirectionLength = std::tan(horizontalFieldOfView / 2) * m_forwardDirectionLength;
        m_upDirectionLength = m_rightDirectionLength / aspectRatio;
        m_upDirection = GetNormalizedUpDirection() * m_upDirectionLength;
        m_rightDirection = GetNormalizedRightDirection() * m_rightDirectionLength;
    }

    void SetLens(float horizontalFieldOfView, float aspectRatio, float nearDepth, float farDepth = std::numeric_limits<float>::infinity())
    {
        SetLens(horizontalFieldOfView, aspectRatio);
        m_nearDepth = nearDepth;
        m_farDepth = farDepth;
    }

    // The camera block of App::Impl::Update (Source/App.cpp:531-553), minus the matrices.
    void Fill(Camera& camera, Float2 jitter) const
    {
        camera.IsNormalizedDepthReversed = m_isNormalizedDepthReversed;
        camera.PreviousPosition = camera.Position;
        camera.Position = m_position;
        camera.RightDirection = m_rightDirection;
        camera.UpDirection = m_upDirection;
        camera.ForwardDirection = m_forwardDirection;
        camera.NearDepth = m_nearDepth;
        camera.FarDepth = m_farDepth;
        camera.Jitter = jitter;
    }

    // The matrices of App::Impl::Update (Source/App.cpp:534-551), DirectXMath row-vector layout (clip = [p, 1] . M): WorldToView
    // = XMMatrixLookToLH(position, forward, up); ViewToProjection = left-handed perspective with the lens primary_ray uses
    // (x scale |Forward| / |Right| = 1 / tan(HFOV / 2), y scale |Forward| / |Up| = that times the aspect ratio, from the stored
    // directions so that a primary hit projects back onto its own pixel), depth [0, 1] or reversed, finite or infinite far as
    // Camera.ixx:146-153 selects.  Unlike Camera.ixx's SetLens(h, a, near, far), which builds the projection before it stores the new
    // depths, the projection here always uses the NearDepth / FarDepth the camera carries (spec S12).  The Previous* matrices are
    // those of `previous`, the camera of the previous frame (itself filled by FillMatrices).
    void FillMatrices(Camera& camera, const Camera& previous) const
    {
        Matrices m;
        Current(m);
        // the previous frame's WorldToView / ViewToProjection are the inverses of what its camera carries
        M4 pv2w, pp2v, pw2v, pv2p;
        Load(previous.Matrices[7], pv2w);
        Load(previous.Matrices[6], pp2v);
        Invert(pv2w, pw2v);
        Invert(pp2v, pv2p);
        Store(pw2v, camera.Matrices[0]);                                        // PreviousWorldToView
        Store(pv2p, camera.Matrices[1]);                                        // PreviousViewToProjection
        std::memcpy(camera.Matrices[2], previous.Matrices[5], sizeof(float) * 16);  // PreviousWorldToProjection
        std::memcpy(camera.Matrices[3], previous.Matrices[6], sizeof(float) * 16);  // PreviousProjectionToView
        std::memcpy(camera.Matrices[4], previous.Matrices[7], sizeof(float) * 16);  // PreviousViewToWorld
        StoreCurrent(m, camera);
    }

    // A first frame (no previous camera): the Previous* matrices are this frame's own, so a resting view has no motion.
    void FillMatrices(Camera& camera) const
    {
        Matrices m;
        Current(m);
        Store(m.w2v, camera.Matrices[0]);  // PreviousWorldToView
        Store(m.v2p, camera.Matrices[1]);  // PreviousViewToProjection
        Store(m.w2p, camera.Matrices[2]);  // PreviousWorldToProjection
        Store(m.p2v, camera.Matrices[3]);  // PreviousProjectionToView
        Store(m.v2w, camera.Matrices[4]);  // PreviousViewToWorld
        StoreCurrent(m, camera);
    }

private:
    using M4 = double[4][4];
    struct Matrices { M4 w2v, v2w, v2p, p2v, w2p; };

    // this frame's WorldToView, ViewToWorld, ViewToProjection, ProjectionToView and WorldToProjection, in double
    void Current(Matrices& m) const
    {
        const Float3 r = GetNormalizedRightDirection(), u = GetNormalizedUpDirection(), f = GetNormalizedForwardDirection();
        {
            // XMMatrixLookToLH: R2 = normalize(forward), R0 = normalize(cross(up, R2)), R1 = cross(R2, R0)
            const Float3 r2 = f, r0 = detail::Normalized(detail::Cross(m_upDirection, r2)), r1 = detail::Cross(r2, r0);
            const Float3 R[3] = { r0, r1, r2 };
            for (int k = 0; k < 3; k++) {
                m.w2v[0][k] = R[k].x; m.w2v[1][k] = R[k].y; m.w2v[2][k] = R[k].z;
                m.w2v[3][k] = -((double)R[k].x * m_position.x + (double)R[k].y * m_position.y + (double)R[k].z * m_position.z);
                m.w2v[k][3] = 0;
            }
            m.w2v[3][3] = 1;
        }
        {
            // SimpleMath Matrix(right, up, forward) with the position in row 3 (Camera.ixx:120-124)
            const Float3 R[3] = { r, u, f };
            for (int k = 0; k < 3; k++) { m.v2w[k][0] = R[k].x; m.v2w[k][1] = R[k].y; m.v2w[k][2] = R[k].z; m.v2w[k][3] = 0; }
            m.v2w[3][0] = m_position.x; m.v2w[3][1] = m_position.y; m.v2w[3][2] = m_position.z; m.v2w[3][3] = 1;
        }
        {
            // the lens as the stored (float) directions carry it: |Forward| / |Right| = 1 / tan(HFOV / 2), |Forward| / |Up| = that times the aspect
            const auto len = [](const Float3& v) { return std::sqrt((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z); };
            const double xs = len(m_forwardDirection) / len(m_rightDirection), ys = len(m_forwardDirection) / len(m_upDirection);
            const double n = m_nearDepth, fd = m_farDepth;
            const bool inf = std::isinf(m_farDepth);
            double a, b;
            if (m_isNormalizedDepthReversed) { a = inf ? 0.0 : n / (n - fd); b = inf ? n : -n * fd / (n - fd); }
            else { a = inf ? 1.0 : fd / (fd - n); b = inf ? -n : -n * fd / (fd - n); }
            for (auto& row : m.v2p) for (double& x : row) x = 0;
            m.v2p[0][0] = xs; m.v2p[1][1] = ys; m.v2p[2][2] = a; m.v2p[2][3] = 1; m.v2p[3][2] = b;
        }
        Invert(m.v2p, m.p2v);
        Multiply(m.w2v, m.v2p, m.w2p);
    }
    static void StoreCurrent(const Matrices& m, Camera& camera)
    {
        Store(m.w2p, camera.Matrices[5]);  // WorldToProjection
        Store(m.p2v, camera.Matrices[6]);  // ProjectionToView
        Store(m.v2w, camera.Matrices[7]);  // ViewToWorld
    }
    static void Load(const float* m, double (&o)[4][4]) { for (int i = 0; i < 16; i++) o[i / 4][i % 4] = m[i]; }
    static void Store(const double (&m)[4][4], float* o) { for (int i = 0; i < 16; i++) o[i] = static_cast<float>(m[i / 4][i % 4]); }
    static void Multiply(const double (&a)[4][4], const double (&b)[4][4], double (&o)[4][4])
    {
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) o[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] + a[i][3] * b[3][j];
    }
    // Gauss-Jordan with partial pivoting (every matrix here is invertible: a rigid transform or a perspective projection)
    static void Invert(const double (&m)[4][4], double (&o)[4][4])
    {
        double a[4][8];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) { a[i][j] = m[i][j]; a[i][j + 4] = i == j ? 1 : 0; }
        for (int c = 0; c < 4; c++) {
            int p = c;
            for (int i = c + 1; i < 4; i++) if (std::fabs(a[i][c]) > std::fabs(a[p][c])) p = i;
            for (int j = 0; j < 8; j++) std::swap(a[c][j], a[p][j]);
            const double inv = 1.0 / a[c][c];
            for (int j = 0; j < 8; j++) a[c][j] *= inv;
            for (int i = 0; i < 4; i++)
                if (i != c && a[i][c] != 0) { const double k = a[i][c]; for (int j = 0; j < 8; j++) a[i][j] -= k * a[c][j]; }
        }
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) o[i][j] = a[i][j + 4];
    }

    bool m_isNormalizedDepthReversed;
    float m_rightDirectionLength = 1, m_upDirectionLength = 1, m_forwardDirectionLength = 1;
    Float3 m_position, m_rightDirection{ 1, 0, 0 }, m_upDirection{ 0, 1, 0 }, m_forwardDirection{ 0, 0, 1 };
    Quaternion m_rotation;
    float m_horizontalFieldOfView{}, m_aspectRatio{}, m_nearDepth = 1e-2f, m_farDepth = std::numeric_limits<float>::infinity();
};

}  // namespace dxrs
