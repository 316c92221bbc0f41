// physics_host.cpp -- TEST SHIM: csrc/pt_physics.h (row N23, DESIGN.md spec S27) compiled as plain host C++ (the flags of sharc_ff_host.cpp),
// so that the tests can check every rule without a GPU and the GPU state against it bit for bit.  Not part of the product; never loaded by it.
#include "physics_host.h"

using namespace phhost;

extern "C" {

void* ph_host_create(const PtSphere* spheres, const PtPhysicsBody* bodies, const float* lin_vel, const float* ang_vel, const float* rotations, uint32_t n)
{
    State* st = new State;
    st->set(spheres, bodies, lin_vel, ang_vel, rotations, n);
    return st;
}

void ph_host_destroy(void* h) { delete static_cast<State*>(h); }

// pt_physics_step: `substeps` steps of dt / substeps; report = {Contacts, Clamped, Frozen, Steps}
void ph_host_step(void* h, const PtPhysicsSettings* s, const PtPhysicsAttractor* attractors, uint32_t n_attractors, float dt, uint32_t substeps, uint32_t* report)
{
    State& st = *static_cast<State*>(h);
    const PhParams p = make_params(*s, attractors, n_attractors, dt / (float)substeps);
    uint32_t r[3] = { 0, 0, 0 };
    for (uint32_t k = 0; k < substeps; k++) step(st, *s, p, r);
    report[0] = r[0]; report[1] = r[1]; report[2] = r[2]; report[3] = (uint32_t)st.steps;
}

// pt_physics_download, plus the bodies' flags and the pairs S27.4 did not give to exactly one handler
void ph_host_download(void* h, float* spheres, float* rotations, float* lin_vel, float* ang_vel, uint32_t* flags, uint32_t* rule_violations)
{
    const State& st = *static_cast<State*>(h);
    for (uint32_t i = 0; i < st.n; i++) {
        if (spheres) { spheres[4 * i] = st.sph[i].x; spheres[4 * i + 1] = st.sph[i].y; spheres[4 * i + 2] = st.sph[i].z; spheres[4 * i + 3] = st.sph[i].w; }
        if (rotations) { rotations[4 * i] = st.rot[i].x; rotations[4 * i + 1] = st.rot[i].y; rotations[4 * i + 2] = st.rot[i].z; rotations[4 * i + 3] = st.rot[i].w; }
        if (lin_vel) { lin_vel[3 * i] = st.vel[i].x; lin_vel[3 * i + 1] = st.vel[i].y; lin_vel[3 * i + 2] = st.vel[i].z; }
        if (ang_vel) { ang_vel[3 * i] = st.ang[i].x; ang_vel[3 * i + 1] = st.ang[i].y; ang_vel[3 * i + 2] = st.ang[i].z; }
        if (flags) flags[i] = st.body[i].Flags;
    }
    if (rule_violations) *rule_violations = st.rule_violations;
}

// n pairs through ph_pair_impulse.  in: 28 floats per pair = sa(4) sb(4) va wa vb wb v0a v0b (3 each) ima imb; counts: na, nb per pair;
// prm: h, e, mu, beta, slop, threshold.  out: 14 floats per pair = dva dwa dvb dwb lambda jt; hit[i] = the function's result
void ph_host_pairs(const float* in, const uint32_t* counts, uint32_t n, const float* prm, float* out, uint32_t* hit)
{
    PhParams p{};
    p.h = prm[0]; p.restitution = prm[1]; p.friction = prm[2]; p.baumgarte = prm[3]; p.slop = prm[4]; p.bounce_threshold = prm[5];
    for (uint32_t i = 0; i < n; i++) {
        const float* f = in + 28 * i;
        PhPair q;
        q.sa = { f[0], f[1], f[2], f[3] }; q.sb = { f[4], f[5], f[6], f[7] };
        q.va = make_f3(f[8], f[9], f[10]); q.wa = make_f3(f[11], f[12], f[13]); q.vb = make_f3(f[14], f[15], f[16]); q.wb = make_f3(f[17], f[18], f[19]);
        q.v0a = make_f3(f[20], f[21], f[22]); q.v0b = make_f3(f[23], f[24], f[25]);
        q.ima = f[26]; q.imb = f[27];
        q.na = counts[2 * i]; q.nb = counts[2 * i + 1];
        PhImpulse r{};
        hit[i] = ph_pair_impulse(q, p, r) ? 1u : 0u;
        float* o = out + 14 * i;
        const f3 v[4] = { r.dva, r.dwa, r.dvb, r.dwb };
        for (int k = 0; k < 4; k++) { o[3 * k] = v[k].x; o[3 * k + 1] = v[k].y; o[3 * k + 2] = v[k].z; }
        o[12] = r.lambda; o[13] = r.jt;
    }
}

// n bodies through ph_integrate.  state: sph(4) rot(4) v(3) w(3) per body, updated in place where ok[i]
void ph_host_integrate(float* state, uint32_t n, float h, uint32_t* ok)
{
    for (uint32_t i = 0; i < n; i++) {
        float* f = state + 14 * i;
        PhVec4 s = { f[0], f[1], f[2], f[3] }, r = { f[4], f[5], f[6], f[7] };
        ok[i] = ph_integrate(s, r, make_f3(f[8], f[9], f[10]), make_f3(f[11], f[12], f[13]), h) ? 1u : 0u;
        f[0] = s.x; f[1] = s.y; f[2] = s.z; f[3] = s.w; f[4] = r.x; f[5] = r.y; f[6] = r.z; f[7] = r.w;
    }
}

void ph_host_quantize(const float* x, uint32_t n, int64_t* q, uint32_t* clamped)
{
    for (uint32_t i = 0; i < n; i++) { bool c = false; q[i] = ph_quantize(x[i], c); clamped[i] = c ? 1u : 0u; }
}

void ph_host_apply(const float* v, const int64_t* acc, uint32_t n, float* out)
{
    for (uint32_t i = 0; i < n; i++) out[i] = ph_apply(v[i], acc[i]);
}

// ph_acceleration of every body of (spheres, bodies) under the attractors: out = n * 3
void ph_host_acceleration(const float* spheres, const PtPhysicsBody* bodies, uint32_t n, const PtPhysicsAttractor* attractors, uint32_t n_attractors, float* out)
{
    PtPhysicsSettings s{};
    const PhParams p = make_params(s, attractors, n_attractors, 1.0f);
    for (uint32_t i = 0; i < n; i++) {
        const f3 a = ph_acceleration(reinterpret_cast<const PhVec4*>(spheres), i, bodies[i], p);
        out[3 * i] = a.x; out[3 * i + 1] = a.y; out[3 * i + 2] = a.z;
    }
}

}  // extern "C"
