// pt_beam_cache.h -- the host half of the primary beams (DESIGN.md "Primary beams"): which later camera poses may use the lists that
// pt_beam.h's pyramids were walked for, and how a moving camera's next lists are planned.  Host-only double arithmetic on plain floats: no
// HIP types, no PtContext.  pt_api.hip beam_cache_lookup keeps the state (buffers, events, shares) and calls these;
// tests/hostshim/beam_host.cpp compiles them for tests/test_primary_beams.py, which checks every accepted pose's rays against the pyramids.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pt {

inline double beam_len3(const float* v) { return std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }

inline double beam_dist(const float* a, const float* b)
{
    const double dx = (double)a[0] - b[0], dy = (double)a[1] - b[1], dz = (double)a[2] - b[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz);
}

// What the pixel bounds below need of a lens: the image size and the lengths of the camera's axes (Right, Up, Forward).
struct BeamLens {
    double f_px;          // the focal length in pixels (the larger of the two for pixels that are not square)
    double corner;        // the image corner's angle off the view axis
    double half_diag_px;  // half the image's diagonal
};

inline BeamLens beam_lens(uint32_t img_w, uint32_t img_h, double len_r, double len_u, double len_f)
{
    BeamLens l;
    const double fx_px = 0.5 * (double)img_w * len_f / len_r, fy_px = 0.5 * (double)img_h * len_f / len_u;  // (equal for square pixels)
    l.f_px = std::max(fx_px, fy_px);
    l.corner = std::atan(std::sqrt(len_r * len_r + len_u * len_u) / len_f);
    l.half_diag_px = 0.5 * std::sqrt((double)img_w * img_w + (double)img_h * img_h);
    return l;
}

// The rotation that takes orientation p to orientation q (both with this lens; 9 floats each: Right, Up, Forward) as a rotation vector
// (axis * angle): R = Q * P^T over the normalised axes; angle from the trace, axis from the antisymmetric part.  R is a rotation only when
// both bases are orthogonal and of one handedness: beam_within checks that before it trusts the angle.
inline double beam_rotation_between(const float* p, const float* q, double w[3])
{
    double R[3][3] = {};
    for (int k = 0; k < 3; k++) {
        const double lp = beam_len3(p + 3 * k), lq = beam_len3(q + 3 * k), inv = lp > 0.0 && lq > 0.0 ? 1.0 / (lp * lq) : 0.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] += (double)q[3 * k + i] * (double)p[3 * k + j] * inv;
    }
    const double ax[3] = { R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1] };  // 2 sin(angle) * axis
    const double s2 = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), c2 = R[0][0] + R[1][1] + R[2][2] - 1.0;  // 2 sin, 2 cos
    const double angle = std::atan2(s2, c2);
    for (int i = 0; i < 3; i++) w[i] = s2 > 0.0 ? ax[i] / s2 * angle : 0.0;
    return angle;  // in [0, pi]; a half turn has no axis here, and nothing builds lists for one
}

// How far, in pixels, a ray's crossing of the image can move when the camera turns by `angle` (any axis): a direction moves by at most that
// angle, and at an angle a off the view axis a change of direction moves the crossing by at most f / cos^2(a) pixels per radian (f = the focal
// length in pixels) -- taken at the image corner, plus the turn itself.
inline double beam_turn_px(const BeamLens& l, double angle)
{
    const double a = std::min(l.corner + angle, 1.55), cs = std::cos(a);
    return angle * l.f_px / (cs * cs) * 1.01;
}

// ... and when its axes' lengths differ (by rounding: relative differences times the image's half diagonal, with the tangent at the corner)
inline double beam_lens_px(const BeamLens& l, const float* p, const float* q)
{
    double worst = 0.0;
    for (int k = 0; k < 3; k++) {
        const double lp = beam_len3(p + 3 * k), lq = beam_len3(q + 3 * k);
        worst = std::max(worst, lp > 0.0 && lq > 0.0 ? std::fabs(lq / lp - 1.0) : 1e30);
    }
    const double cs = std::cos(std::min(l.corner, 1.55));
    return 2.0 * worst * l.half_diag_px / (cs * cs) * 1.01;
}

// Two calls show one view (whatever the pose) when their lenses differ by at most this many pixels
constexpr double kBeamSameLensPx = 0.02;
inline bool beam_same_lens(const BeamLens& l, const float* p, const float* q) { return beam_lens_px(l, p, q) <= kBeamSameLensPx; }

// How far a basis is from orthogonal: the sum of the absolute cosines between its axes (NaN for a zero or non-finite axis)
inline double beam_skew(const float* p)
{
    const double l0 = beam_len3(p), l1 = beam_len3(p + 3), l2 = beam_len3(p + 6);
    auto dotd = [&](int a, int b) { return (double)p[3 * a] * p[3 * b] + (double)p[3 * a + 1] * p[3 * b + 1] + (double)p[3 * a + 2] * p[3 * b + 2]; };
    return std::fabs(dotd(0, 1)) / (l0 * l1) + std::fabs(dotd(0, 2)) / (l0 * l2) + std::fabs(dotd(1, 2)) / (l1 * l2);
}

// Right . (Up x Forward): its sign is the basis' handedness
inline double beam_triple(const float* p)
{
    const double r[3] = { p[0], p[1], p[2] }, u[3] = { p[3], p[4], p[5] }, f[3] = { p[6], p[7], p[8] };
    return r[0] * (u[1] * f[2] - u[2] * f[1]) + r[1] * (u[2] * f[0] - u[0] * f[2]) + r[2] * (u[0] * f[1] - u[1] * f[0]);
}

// A basis whose axes' cosines add up to more than this serves bit-identical poses only (an off-axis camera: Forward not at right angles)
constexpr double kBeamMaxSkew = 1e-3;

// May a frame at pose q (position, basis) use the lists walked for pose b with this slack and margin?  Yes when q's position lies within
// the slack and every pixel ray of q crosses b's image plane within margin_px pixels of where b's ray of that pixel does.
// Bit-identical bases: always.  Otherwise the displacement is bounded as a turn plus a change of the axes' lengths, which is sound only
// for bases that are rotations of one another: both orthogonal, of one handedness (a mirrored basis has R = I - 2 r r^T: symmetric,
// trace 1, "angle" 0).  Axes that are orthogonal to rounding only -- cosines c, summing to s for both bases -- are within 0.71 s
// (half the norm of the Gram matrix's off-diagonal part) of orthonormal ones; that moves each camera's rays by at most 0.75 s
// radians and the angle read from R by at most 0.87 s (|d ax| <= sqrt(6) |d R|, angle ~ |ax| / 2): 2 s added to the angle covers both.
// A sheared basis (Forward + eps * Right: R's antisymmetric part holds eps / 2 where the rays move by eps) passes only while 2 s >= eps
// pays for it, and not at all beyond kBeamMaxSkew, where the first-order argument ends.
inline bool beam_within(const BeamLens& l, const float* b_pos, const float* b_basis, float slack, float margin_px, const float* q_pos, const float* q_basis)
{
    if (slack == 0.0f ? std::memcmp(b_pos, q_pos, 12) != 0 : beam_dist(b_pos, q_pos) > (double)slack * (1.0 - 1e-4)) return false;
    if (std::memcmp(b_basis, q_basis, 36) == 0) return true;
    if (margin_px == 0.0f) return false;
    const double skew = beam_skew(b_basis) + beam_skew(q_basis);
    if (!(skew <= kBeamMaxSkew)) return false;  // (NaN: a zero or non-finite axis)
    if (!(beam_triple(b_basis) * beam_triple(q_basis) > 0.0)) return false;
    double w[3];
    return beam_turn_px(l, beam_rotation_between(b_basis, q_basis, w) + 2.0 * skew) + beam_lens_px(l, b_basis, q_basis) <= (double)margin_px * (1.0 - 1e-3);
}

// The pose f frames ahead of (pos, basis) for a camera that keeps its velocity v (per frame) and its turn (rotation vector `turn` of
// angle `turned` per frame): the axes turned by f times the last turn (Rodrigues), their lengths kept
inline void beam_ahead(const float* pos, const double v[3], const float* basis, const double turn[3], double turned, double f, float out_pos[3], float out_basis[9])
{
    for (int i = 0; i < 3; i++) out_pos[i] = (float)((double)pos[i] + f * v[i]);
    const double ang = f * turned;
    std::memcpy(out_basis, basis, 36);
    if (ang > 0.0 && turned > 0.0) {
        const double k[3] = { turn[0] / turned, turn[1] / turned, turn[2] / turned }, cs = std::cos(ang), sn = std::sin(ang);
        for (int x = 0; x < 3; x++) {
            const double p[3] = { basis[3 * x], basis[3 * x + 1], basis[3 * x + 2] };
            const double kxp[3] = { k[1] * p[2] - k[2] * p[1], k[2] * p[0] - k[0] * p[2], k[0] * p[1] - k[1] * p[0] }, kp = k[0] * p[0] + k[1] * p[1] + k[2] * p[2];
            for (int i = 0; i < 3; i++) out_basis[3 * x + i] = (float)(p[i] * cs + kxp[i] * sn + k[i] * kp * (1.0 - cs));
        }
    }
}

// A moving camera's next lists.  They are built in shares inside the primary passes of the next n_build frames, are readable `lanes` calls
// after the last share, and are made for the `span` frames from then on: centred on the position -- and turned to the orientation --
// extrapolated to the middle of that span (beam_ahead by centre_ahead frames), with half the span's travel, two frames' and what the
// velocity's last change (acc) would add up to by the span's last frame as slack, and the same of the turn, in pixels, as margin.
// span starts at `reach` and shrinks until the slack fits max_slack and the margin max_margin; below 4 frames nothing is built.
struct BeamPlan {
    double span;          // frames the lists are made for; < 4: no build
    double centre_ahead;  // how many frames ahead of this one the lists' pose lies
    float slack, margin_px;
};

inline BeamPlan beam_plan(const BeamLens& l, double step, double acc, double turned, double turn_acc, double n_build, double lanes, double reach, double max_slack, double max_margin)
{
    // (a velocity that goes on changing by acc per frame has added acc * e (e + 1) / 2 by frame e, the span's last: the lists' centre is
    // extrapolated with the velocity of this frame alone)
    auto drift = [&](double sp) { const double e = n_build + lanes + sp; return 0.5 * e * (e + 1.0); };
    auto slack_for = [&](double sp) { return (0.5 * sp + 2.0) * step + acc * drift(sp); };
    auto margin_for = [&](double sp) { return turned > 0.0 || turn_acc > 0.0 ? beam_turn_px(l, (0.5 * sp + 2.0) * turned + turn_acc * drift(sp)) + 0.05 : 0.0; };
    BeamPlan p{};
    p.span = reach;
    while (p.span >= 4.0 && (slack_for(p.span) > max_slack || margin_for(p.span) > max_margin)) p.span -= 2.0;
    if (!(p.span >= 4.0)) return p;
    p.slack = (float)slack_for(p.span);
    p.margin_px = (float)margin_for(p.span);
    p.centre_ahead = n_build - 1.0 + lanes + 0.5 * p.span;
    return p;
}

}  // namespace pt
