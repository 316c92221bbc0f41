// pt_api_post.hip -- the entry points of the C-ABI (include/pt_api.h) that touch nothing but the context's stream and their own state:
// tone mapping, accumulation, bloom, the NRD composition and stand-in, super-resolution, sharpening, chromatic aberration, frame
// interpolation and ray reconstruction.
// Everything that knows lanes, the scene, the tree or the beam cache is in pt_api.hip and pt_api_side.hip (the side passes of a frame).
#include <algorithm>
#include <string>

#include "pt_context.h"
#include "pt_bloom.h"
#include "pt_nrd.h"
#include "pt_denoise.h"
#include "pt_reblur.h"
#include "pt_upscale.h"
#include "pt_nis.h"
#include "pt_chromab.h"
#include "pt_framegen.h"
#include "pt_rr.h"

namespace {

// Row N9's history and work buffers per pixel: two history slots of four float4 (accumulated diffuse / specular, moments, guide), two
// hit distances, two a-trous ping-pong pairs of float4.
constexpr uint64_t kDnBytesPerPixel = 2 * 4 * sizeof(float4) + 2 * sizeof(float) + 4 * sizeof(float4);
// Row N30's history and work buffers per pixel: two history slots of five float4 (slow diffuse / specular, fast diffuse / specular,
// guide) and two work float4.
constexpr uint64_t kRbBytesPerPixel = 2 * 5 * sizeof(float4) + 2 * sizeof(float4);
// Row N11's history per output pixel and slot: a float4 (t-space colour, accumulated weight) and a float (depth).
constexpr uint64_t kUpSlotBytesPerPixel = sizeof(float4) + sizeof(float);
// Row N15's history per output pixel and slot: two float4 (t-space colour + weight, normal + roughness) and a float (depth); its
// prepare pass's records per render pixel: three float4.
constexpr uint64_t kRrSlotBytesPerPixel = 2 * sizeof(float4) + sizeof(float), kRrRecordBytesPerPixel = 3 * sizeof(float4);

// The two-slot history of a pass (PtContext::dn, up, fg).  history_begin: allocated on first use and again when `dims` change -- the
// history is only used on `stream`, so once the calls queued there have finished the old one is free (the render lanes never touch it,
// their frames in flight go on); a new allocation restarts the history.  A failure leaves no memory and valid == false.
PtStatus history_begin(PtContext* c, History& H, const uint32_t (&dims)[4], uint64_t bytes, bool& restart)
{
    if (H.mem && std::equal(dims, dims + 4, H.dims)) return PT_OK;
    if (H.mem) PT_HIP(c, hipStreamSynchronize(c->stream));
    free_dev(H.mem);
    H.valid = false;
    std::fill(H.dims, H.dims + 4, 0u);
    PT_HIP(c, hipMalloc(&H.mem, bytes));
    std::copy(dims, dims + 4, H.dims);
    restart = true;
    return PT_OK;
}

// ... and once the call's launches have been queued: the slot it wrote becomes the previous one
void history_commit(History& H, uint64_t tag)
{
    H.slot ^= 1u;
    H.tag = tag;
    H.valid = true;
}

}  // namespace

extern "C" {

PtStatus pt_tonemap(PtContext* c, const void* hdr, uint32_t n_pixels, const PtToneMapParams* params, void* out)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!hdr || !out || !params) return fail(c, PT_ERR_INVALID_ARG, "pt_tonemap: null pointer");
    if (params->Operator > kToneACESFilmic || params->TransferFunction > kTransferST2084 || params->ColorRotation > kRotate709toP3D65)
        return fail(c, PT_ERR_INVALID_ARG, "pt_tonemap: unknown operator / transfer function / colour rotation");
    if (n_pixels == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, launch_tonemap(static_cast<const float4*>(hdr), static_cast<uint32_t*>(out), n_pixels, *params, c->stream));
    return PT_OK;
}

PtStatus pt_accumulate(PtContext* c, void* accum, const void* radiance, uint32_t n_pixels, uint32_t frames_accumulated)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!accum || !radiance) return fail(c, PT_ERR_INVALID_ARG, "pt_accumulate: null pointer");
    if (frames_accumulated == 0xFFFFFFFFu) return fail(c, PT_ERR_INVALID_ARG, "pt_accumulate: frame count overflow");
    if (n_pixels == 0) return PT_OK;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, launch_accumulate(static_cast<float4*>(accum), static_cast<const float4*>(radiance), n_pixels, frames_accumulated, c->stream));
    return PT_OK;
}

PtStatus pt_bloom(PtContext* c, const void* hdr, void* out, uint32_t width, uint32_t height, float strength)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!hdr || !out) return fail(c, PT_ERR_INVALID_ARG, "pt_bloom: null pointer");
    // >= 32: every level of the 5-mip half-size chain is at least one texel; <= 16384: the largest D3D12 2-D texture
    if (width < kBloomMinSize || height < kBloomMinSize || width > 16384u || height > 16384u)
        return fail(c, PT_ERR_INVALID_ARG, "pt_bloom: width and height must be in [32, 16384]");
    if (!(strength >= 0.0f && strength <= 1.0f)) return fail(c, PT_ERR_INVALID_ARG, "pt_bloom: strength must be in [0, 1]");
    PT_HIP(c, hipSetDevice(c->device));
    const uint64_t need = bloom_chain(width, height).texels;
    if (need > c->cap_bloom) {
        // the chain is only used on `stream`: once the bloom calls queued there have finished, the old one is free (the render
        // lanes never touch it, so their frames in flight go on)
        PT_HIP(c, hipStreamSynchronize(c->stream));
        free_dev(c->d_bloom);
        c->cap_bloom = 0;
        PT_HIP(c, hipMalloc(&c->d_bloom, need * sizeof(float4)));
        c->cap_bloom = need;
    }
    PT_HIP(c, launch_bloom(static_cast<const float4*>(hdr), static_cast<float4*>(out), c->d_bloom, width, height, strength, c->stream));
    return PT_OK;
}

// Row N8 -- the NRD composition pass (DESIGN.md spec S14): one launch of pack or compose on the context's stream
PtStatus pt_nrd_composition(PtContext* c, const PtNrdCompositionConstants* k, const PtNrdCompositionTextures* t)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!k || !t) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_composition: null pointer");
    if (k->Denoiser != kNrdReblur && k->Denoiser != kNrdRelax)
        return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_composition: Denoiser must be 2 (NRDReBLUR) or 3 (NRDReLAX)");
    const uint32_t w = k->RenderSize[0], h = k->RenderSize[1];
    if (w == 0 || h == 0 || w > 16384u || h > 16384u) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_composition: RenderSize must be in [1, 16384]");
    const bool pack = k->Pack != 0, reblur = k->Denoiser == kNrdReblur;
    const uint64_t n = (uint64_t)w * h;
    // the buffers this direction uses; a buffer the pass writes must not share a byte with any other (each lane reads its pixel of a
    // written buffer before it writes it, so a written buffer may only overlap itself)
    BufferUse use[7];
    uint32_t nu = 0;
    use[nu++] = {t->LinearDepth, n * 4, 4, false, true, "LinearDepth"};
    use[nu++] = {t->DiffuseAlbedo, n * 12, 4, false, true, "DiffuseAlbedo"};
    use[nu++] = {t->SpecularAlbedo, n * 12, 4, false, true, "SpecularAlbedo"};
    if (pack) {
        if (reblur) use[nu++] = {t->NormalRoughness, n * 16, 16, false, true, "NormalRoughness"};
        use[nu++] = {t->NoisyDiffuse, n * 16, 16, true, true, "NoisyDiffuse"};
        use[nu++] = {t->NoisySpecular, n * 16, 16, true, true, "NoisySpecular"};
    } else {
        use[nu++] = {t->DenoisedDiffuse, n * 16, 16, false, true, "DenoisedDiffuse"};
        use[nu++] = {t->DenoisedSpecular, n * 16, 16, false, true, "DenoisedSpecular"};
        use[nu++] = {t->Radiance, n * 16, 16, true, true, "Radiance"};
    }
    if (const PtStatus st = buffers_ok(c, "pt_nrd_composition", use, nu); st != PT_OK) return st;
    NrdBuffers b{};
    b.linear_depth = static_cast<const float*>(t->LinearDepth);
    b.diffuse_albedo = static_cast<const float*>(t->DiffuseAlbedo);
    b.specular_albedo = static_cast<const float*>(t->SpecularAlbedo);
    if (pack) {
        b.normal_roughness = reblur ? static_cast<const float4*>(t->NormalRoughness) : nullptr;
        b.noisy_diffuse = static_cast<float4*>(t->NoisyDiffuse);
        b.noisy_specular = static_cast<float4*>(t->NoisySpecular);
    } else {
        b.denoised_diffuse = static_cast<const float4*>(t->DenoisedDiffuse);
        b.denoised_specular = static_cast<const float4*>(t->DenoisedSpecular);
        b.radiance = static_cast<float4*>(t->Radiance);
    }
    const NrdHitDistParams P{k->ReBLURHitDistance[0], k->ReBLURHitDistance[1], k->ReBLURHitDistance[2], k->ReBLURHitDistance[3]};
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, launch_nrd_composition(b, (uint32_t)n, pack, k->Denoiser, P, c->stream));
    return PT_OK;
}

// Row N9 -- the NRD stand-in (DESIGN.md spec S15): pass (a), pass (b) and the a-trous steps on the context's stream, the history
// in the context (kDnBytesPerPixel).
PtStatus pt_nrd_denoise(PtContext* c, const PtNrdDenoiseSettings* s, const PtNrdDenoiseTextures* t)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s || !t) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_denoise: null pointer");
    if (s->Denoiser != kNrdReblur && s->Denoiser != kNrdRelax)
        return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_denoise: Denoiser must be 2 (NRDReBLUR) or 3 (NRDReLAX)");
    if (s->AccumulationMode > 2) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_denoise: AccumulationMode must be 0, 1 or 2");
    const uint32_t w = s->RenderSize[0], h = s->RenderSize[1];
    if (w == 0 || h == 0 || w > 16384u || h > 16384u) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_denoise: RenderSize must be in [1, 16384]");
    if (s->AtrousIterations > kDnMaxIterations) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_denoise: AtrousIterations must be at most 8");
    const uint64_t n = (uint64_t)w * h;
    // an output must not share a byte with any input or the other output (the passes read their neighbours' inputs)
    const BufferUse use[8] = {
        {t->ViewZ, n * 4, 4, false, true, "ViewZ"}, {t->MotionVector, n * 12, 4, false, true, "MotionVector"},
        {t->NormalRoughness, n * 16, 16, false, true, "NormalRoughness"}, {t->BaseColorMetalness, n * 16, 16, false, false, "BaseColorMetalness"},
        {t->InDiffuse, n * 16, 16, false, true, "InDiffuse"}, {t->InSpecular, n * 16, 16, false, true, "InSpecular"},
        {t->OutDiffuse, n * 16, 16, true, true, "OutDiffuse"}, {t->OutSpecular, n * 16, 16, true, true, "OutSpecular"},
    };
    if (const PtStatus st = buffers_ok(c, "pt_nrd_denoise", use, 8); st != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    bool restart = s->AccumulationMode != 0 || !c->dn.valid || c->dn.tag != s->Denoiser;
    if (const PtStatus st = history_begin(c, c->dn, {w, h}, n * kDnBytesPerPixel, restart); st != PT_OK) return st;
    float4* f4 = static_cast<float4*>(c->dn.mem);
    float4* slots[2][4];
    for (int k = 0; k < 2; k++)
        for (int j = 0; j < 4; j++) slots[k][j] = f4 + (uint64_t)(4 * k + j) * n;
    float4* x = f4 + 8 * n;
    const uint32_t cur = c->dn.slot ^ 1u, prev = c->dn.slot;
    DnBuffers b{};
    b.w = w;
    b.h = h;
    b.viewz = static_cast<const float*>(t->ViewZ);
    b.mv = static_cast<const float*>(t->MotionVector);
    b.nr = static_cast<const float4*>(t->NormalRoughness);
    b.in_d = static_cast<const float4*>(t->InDiffuse);
    b.in_s = static_cast<const float4*>(t->InSpecular);
    b.out_d = static_cast<float4*>(t->OutDiffuse);
    b.out_s = static_cast<float4*>(t->OutSpecular);
    b.prev_sig_d = slots[prev][0]; b.prev_sig_s = slots[prev][1]; b.prev_mom = slots[prev][2]; b.prev_guide = slots[prev][3];
    b.sig_d = slots[cur][0]; b.sig_s = slots[cur][1]; b.mom = slots[cur][2]; b.guide = slots[cur][3];
    b.xd[0] = x; b.xs[0] = x + n; b.xd[1] = x + 2 * n; b.xs[1] = x + 3 * n;
    b.hitd = reinterpret_cast<float*>(x + 4 * n);
    DnParams P{};
    P.max_d = s->MaxDiffuseFrames ? s->MaxDiffuseFrames : kDnDefaultFrames;
    P.max_s = s->MaxSpecularFrames ? s->MaxSpecularFrames : kDnDefaultFrames;
    P.restart = restart ? 1u : 0u;
    const uint32_t iterations = s->AtrousIterations ? s->AtrousIterations : kDnDefaultIterations;
    PT_HIP(c, launch_nrd_denoise(b, s->Denoiser, P, iterations, c->stream));
    history_commit(c->dn, s->Denoiser);
    return PT_OK;
}

// Row N30 -- the ReBLUR stand-in (DESIGN.md spec S32): passes (a) to (d) on the context's stream, the history in the context
// (kRbBytesPerPixel), apart from pt_nrd_denoise's.
PtStatus pt_nrd_reblur(PtContext* c, const PtNrdReblurSettings* s, const PtNrdDenoiseTextures* t)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s || !t) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_reblur: null pointer");
    if (s->AccumulationMode > 2) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_reblur: AccumulationMode must be 0, 1 or 2");
    const uint32_t w = s->RenderSize[0], h = s->RenderSize[1];
    if (w == 0 || h == 0 || w > 16384u || h > 16384u) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_reblur: RenderSize must be in [1, 16384]");
    RbParams P{};
    P.max_n = s->MaxAccumulatedFrames ? s->MaxAccumulatedFrames : kRbDefaultFrames;
    P.max_fast = s->MaxFastAccumulatedFrames ? s->MaxFastAccumulatedFrames : kRbDefaultFastFrames;
    P.fix_frames = s->HistoryFixFrames ? s->HistoryFixFrames : kRbDefaultFixFrames;
    if (P.max_fast > P.max_n) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_reblur: MaxFastAccumulatedFrames must be at most MaxAccumulatedFrames");
    for (const float r : { s->MinBlurRadius, s->MaxBlurRadius })
        if (!is_finite(r) || !(r >= 0.0f)) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_reblur: MinBlurRadius and MaxBlurRadius must be finite and not negative");
    P.rmin = s->MinBlurRadius != 0.0f ? s->MinBlurRadius : kRbDefaultMinRadius;
    P.rmax = s->MaxBlurRadius != 0.0f ? s->MaxBlurRadius : kRbDefaultMaxRadius;
    if (P.rmax > kRbMaxRadius) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_reblur: MaxBlurRadius must be at most 64");
    if (P.rmin > P.rmax) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_reblur: MinBlurRadius must be at most MaxBlurRadius");
    if (s->_pad[0] || s->_pad[1] || s->_pad[2]) return fail(c, PT_ERR_INVALID_ARG, "pt_nrd_reblur: padding must be 0");
    const uint64_t n = (uint64_t)w * h;
    // an output must not share a byte with any input or the other output (the passes read their neighbours' inputs)
    const BufferUse use[8] = {
        {t->ViewZ, n * 4, 4, false, true, "ViewZ"}, {t->MotionVector, n * 12, 4, false, true, "MotionVector"},
        {t->NormalRoughness, n * 16, 16, false, true, "NormalRoughness"}, {t->BaseColorMetalness, n * 16, 16, false, false, "BaseColorMetalness"},
        {t->InDiffuse, n * 16, 16, false, true, "InDiffuse"}, {t->InSpecular, n * 16, 16, false, true, "InSpecular"},
        {t->OutDiffuse, n * 16, 16, true, true, "OutDiffuse"}, {t->OutSpecular, n * 16, 16, true, true, "OutSpecular"},
    };
    if (const PtStatus st = buffers_ok(c, "pt_nrd_reblur", use, 8); st != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    bool restart = s->AccumulationMode != 0 || !c->rb.valid;  // (a change of RenderSize makes a new allocation, which restarts)
    if (const PtStatus st = history_begin(c, c->rb, {w, h}, n * kRbBytesPerPixel, restart); st != PT_OK) return st;
    // the allocation: per slot slow[2], fast[2], guide; then the work buffers x[2]
    float4* const f4 = static_cast<float4*>(c->rb.mem);
    const uint32_t cur = c->rb.slot ^ 1u, prev = c->rb.slot;
    RbBuffers b{};
    b.w = w;
    b.h = h;
    b.viewz = static_cast<const float*>(t->ViewZ);
    b.mv = static_cast<const float*>(t->MotionVector);
    b.nr = static_cast<const float4*>(t->NormalRoughness);
    b.in_d = static_cast<const float4*>(t->InDiffuse);
    b.in_s = static_cast<const float4*>(t->InSpecular);
    b.out_d = static_cast<float4*>(t->OutDiffuse);
    b.out_s = static_cast<float4*>(t->OutSpecular);
    for (int l = 0; l < 2; l++) {
        b.prev_slow[l] = f4 + (uint64_t)(5 * prev + l) * n;
        b.prev_fast[l] = f4 + (uint64_t)(5 * prev + 2 + l) * n;
        b.slow[l] = f4 + (uint64_t)(5 * cur + l) * n;
        b.fast[l] = f4 + (uint64_t)(5 * cur + 2 + l) * n;
        b.x[l] = f4 + (uint64_t)(10 + l) * n;
    }
    b.prev_guide = f4 + (uint64_t)(5 * prev + 4) * n;
    b.guide = f4 + (uint64_t)(5 * cur + 4) * n;
    P.restart = restart ? 1u : 0u;
    P.frame = s->FrameIndex;
    PT_HIP(c, launch_nrd_reblur(b, P, c->stream));
    history_commit(c->rb, 0);
    return PT_OK;
}

// the slot the last pt_nrd_reblur call wrote, for tests: slow diffuse, slow specular, fast diffuse, fast specular, guide (float4 per
// pixel each; a null pointer skips one).  Waits for the stream.
PtStatus pt_nrd_reblur_history(PtContext* c, void* slow_d, void* slow_s, void* fast_d, void* fast_s, void* guide)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!c->rb.valid || !c->rb.mem) return fail(c, PT_ERR_STATE, "pt_nrd_reblur_history: no pt_nrd_reblur call has been made");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t n = (uint64_t)c->rb.dims[0] * c->rb.dims[1];
    const float4* const f4 = static_cast<const float4*>(c->rb.mem) + (uint64_t)5 * c->rb.slot * n;
    void* const dst[5] = { slow_d, slow_s, fast_d, fast_s, guide };
    for (int k = 0; k < 5; k++)
        if (dst[k]) PT_HIP(c, hipMemcpy(dst[k], f4 + (uint64_t)k * n, n * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

// Row N11 -- the super-resolution stand-in (DESIGN.md spec S17): one launch on the context's stream, the history in the context
// (kUpSlotBytesPerPixel).
PtStatus pt_upscale(PtContext* c, const PtUpscaleSettings* s, const PtUpscaleTextures* t)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s || !t) return fail(c, PT_ERR_INVALID_ARG, "pt_upscale: null pointer");
    const uint32_t w = s->InputSize[0], h = s->InputSize[1], W = s->OutputSize[0], H = s->OutputSize[1];
    if (w == 0 || h == 0 || w > kUpMaxSize || h > kUpMaxSize) return fail(c, PT_ERR_INVALID_ARG, "pt_upscale: InputSize must be in [1, 16384]");
    if (W < w || H < h || W > kUpMaxSize || H > kUpMaxSize || (uint64_t)W > (uint64_t)kUpMaxRatio * w || (uint64_t)H > (uint64_t)kUpMaxRatio * h)
        return fail(c, PT_ERR_INVALID_ARG, "pt_upscale: OutputSize must be in [InputSize, 4 * InputSize] per axis and at most 16384");
    for (const float j : { s->Jitter[0], s->Jitter[1] })
        if (!is_finite(j) || !(pt_abs(j) <= 1.0f)) return fail(c, PT_ERR_INVALID_ARG, "pt_upscale: Jitter must be finite and within [-1, 1]");
    float max_a = s->MaxHistoryWeight;
    if (max_a == 0.0f) max_a = kUpDefaultHistoryWeight;
    if (!is_finite(max_a) || !(max_a >= kUpMinHistoryWeight && max_a <= kUpMaxHistoryWeight))
        return fail(c, PT_ERR_INVALID_ARG, "pt_upscale: MaxHistoryWeight must be 0 or in [1, 256]");
    const uint64_t n_in = (uint64_t)w * h, n_out = (uint64_t)W * H;
    // the output must not share a byte with an input (a workgroup reads the inputs of its neighbours' pixels)
    const BufferUse use[4] = { {t->Color, n_in * 16, 16, false, true, "Color"}, {t->Depth, n_in * 4, 4, false, true, "Depth"},
                               {t->Velocity, n_in * 12, 4, false, true, "Velocity"}, {t->Output, n_out * 16, 16, true, true, "Output"} };
    if (const PtStatus st = buffers_ok(c, "pt_upscale", use, 4); st != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    const uint64_t in_size = (uint64_t)w << 32 | h;  // a change of either size restarts the history
    bool restart = s->Reset != 0 || !c->up.valid || c->up.tag != in_size;
    if (const PtStatus st = history_begin(c, c->up, {W, H}, 2 * n_out * kUpSlotBytesPerPixel, restart); st != PT_OK) return st;
    float4* const hist = static_cast<float4*>(c->up.mem);
    const uint32_t cur = c->up.slot ^ 1u, prev = c->up.slot;
    float* zs = reinterpret_cast<float*>(hist + 2 * n_out);
    UpBuffers b{};
    b.color = static_cast<const float4*>(t->Color);
    b.depth = static_cast<const float*>(t->Depth);
    b.velocity = static_cast<const float*>(t->Velocity);
    b.out = static_cast<float4*>(t->Output);
    b.prev_hist = hist + prev * n_out;
    b.prev_z = zs + prev * n_out;
    b.hist = hist + cur * n_out;
    b.hist_z = zs + cur * n_out;
    const UpParams P = up_params(w, h, W, H, s->Jitter[0], s->Jitter[1], max_a);
    PT_HIP(c, launch_upscale(b, P, restart, c->stream));
    history_commit(c->up, in_size);
    return PT_OK;
}

PtStatus pt_upscale_input_size(uint32_t mode, uint32_t out_w, uint32_t out_h, uint32_t* w, uint32_t* h)
{
    if (!w || !h || mode > kUpModeUltraPerformance || out_w == 0 || out_h == 0) return PT_ERR_INVALID_ARG;
    const uint32_t r10 = up_ratio10(mode == kUpModeAuto ? up_auto_mode(out_w, out_h) : mode);
    *w = up_input_extent(out_w, r10);
    *h = up_input_extent(out_h, r10);
    return PT_OK;
}

// Row N12 -- the sharpening stand-in (DESIGN.md spec S18): one launch on the context's stream, no state
PtStatus pt_nis_sharpen(PtContext* c, const PtNisSettings* s, const PtNisTextures* t)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s || !t) return fail(c, PT_ERR_INVALID_ARG, "pt_nis_sharpen: null pointer");
    const uint32_t w = s->Size[0], h = s->Size[1];
    if (w == 0 || h == 0 || w > kNisMaxSize || h > kNisMaxSize) return fail(c, PT_ERR_INVALID_ARG, "pt_nis_sharpen: Size must be in [1, 16384]");
    if (!(s->Sharpness >= 0.0f && s->Sharpness <= 1.0f)) return fail(c, PT_ERR_INVALID_ARG, "pt_nis_sharpen: Sharpness must be in [0, 1]");
    if (s->HdrMode > kNisHdrPQ) return fail(c, PT_ERR_INVALID_ARG, "pt_nis_sharpen: HdrMode must be 0 (None), 1 (Linear) or 2 (PQ)");
    // the output must not share a byte with the input (a lane reads its neighbours' texels): no in-place call
    const uint64_t bytes = (uint64_t)w * h * sizeof(float4);
    const BufferUse use[2] = { {t->Color, bytes, 16, false, true, "Color"}, {t->Output, bytes, 16, true, true, "Output"} };
    if (const PtStatus st = buffers_ok(c, "pt_nis_sharpen", use, 2); st != PT_OK) return st;
    if (s->HdrMode == kNisHdrPQ) return fail(c, PT_ERR_UNSUPPORTED, "pt_nis_sharpen: HdrMode 2 (PQ) is not built");
    PT_HIP(c, hipSetDevice(c->device));
    const NisConfig k = nis_config(s->Sharpness, s->HdrMode);
    PT_HIP(c, launch_nis(static_cast<const float4*>(t->Color), static_cast<float4*>(t->Output), w, h, k, s->HdrMode, c->stream));
    return PT_OK;
}

// Row N29 -- chromatic aberration (DESIGN.md spec S31): one launch on the context's stream, no state
PtStatus pt_chromatic_aberration(PtContext* c, const PtChromaticAberrationSettings* s, const PtChromaticAberrationTextures* t)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s || !t) return fail(c, PT_ERR_INVALID_ARG, "pt_chromatic_aberration: null pointer");
    const uint32_t w = s->Size[0], h = s->Size[1];
    if (w == 0 || h == 0 || w > kCabMaxSize || h > kCabMaxSize) return fail(c, PT_ERR_INVALID_ARG, "pt_chromatic_aberration: Size must be in [1, 16384]");
    for (const float f : s->FocusUV)
        if (!is_finite(f) || !(f >= 0.0f && f <= 1.0f)) return fail(c, PT_ERR_INVALID_ARG, "pt_chromatic_aberration: FocusUV must be finite and in [0, 1]");
    for (const float k : s->Offsets)
        if (!is_finite(k) || !(pt_abs(k) <= kCabMaxOffset)) return fail(c, PT_ERR_INVALID_ARG, "pt_chromatic_aberration: Offsets must be finite and within [-1/16, 1/16]");
    if (s->_pad) return fail(c, PT_ERR_INVALID_ARG, "pt_chromatic_aberration: padding must be 0");
    // the output must not share a byte with the input (a lane reads other lanes' texels): no in-place call
    const uint64_t bytes = (uint64_t)w * h * sizeof(float4);
    const BufferUse use[2] = { {t->Color, bytes, 16, false, true, "Color"}, {t->Output, bytes, 16, true, true, "Output"} };
    if (const PtStatus st = buffers_ok(c, "pt_chromatic_aberration", use, 2); st != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    const CabConfig k = cab_config(w, h, s->FocusUV, s->Offsets);
    PT_HIP(c, launch_chromab(static_cast<const float4*>(t->Color), static_cast<float4*>(t->Output), w, h, k, c->stream));
    return PT_OK;
}

// Row N13 -- the frame-interpolation stand-in (DESIGN.md spec S19): a clear, a scatter and a gather on the context's stream; the motion
// field and the previous frame's Color and Depth live in the context.  *generated is decided here, before anything is queued.
PtStatus pt_frame_gen(PtContext* c, const PtFrameGenSettings* s, const PtFrameGenTextures* t, uint32_t* generated)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s || !t) return fail(c, PT_ERR_INVALID_ARG, "pt_frame_gen: null pointer");
    const uint32_t w = s->RenderSize[0], h = s->RenderSize[1], W = s->OutputSize[0], H = s->OutputSize[1];
    if (w == 0 || h == 0 || w > kFgMaxSize || h > kFgMaxSize) return fail(c, PT_ERR_INVALID_ARG, "pt_frame_gen: RenderSize must be in [1, 16384]");
    if (W < w || H < h || W > kFgMaxSize || H > kFgMaxSize || (uint64_t)W > (uint64_t)kFgMaxRatio * w || (uint64_t)H > (uint64_t)kFgMaxRatio * h)
        return fail(c, PT_ERR_INVALID_ARG, "pt_frame_gen: OutputSize must be in [RenderSize, 4 * RenderSize] per axis and at most 16384");
    if (s->Format > kFgFormatRGB10A2) return fail(c, PT_ERR_INVALID_ARG, "pt_frame_gen: Format must be 0 (R8G8B8A8_UNORM) or 1 (R10G10B10A2_UNORM)");
    if (s->_pad[0] || s->_pad[1]) return fail(c, PT_ERR_INVALID_ARG, "pt_frame_gen: padding must be 0");
    const uint64_t n_in = (uint64_t)w * h, n_out = (uint64_t)W * H;
    // the output must not share a byte with an input (a lane reads the colour of other lanes' pixels)
    const BufferUse use[4] = { {t->Color, n_out * 4, 4, false, true, "Color"}, {t->Depth, n_in * 4, 4, false, true, "Depth"},
                               {t->MotionVector, n_in * 12, 4, false, true, "MotionVector"}, {t->Output, n_out * 4, 4, true, true, "Output"} };
    if (const PtStatus st = buffers_ok(c, "pt_frame_gen", use, 4); st != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    bool restart = s->Reset != 0 || !c->fg.valid || c->fg.tag != s->Format;
    if (const PtStatus st = history_begin(c, c->fg, {w, h, W, H}, n_in * 8 + 2 * n_out * 4 + 2 * n_in * 4, restart); st != PT_OK) return st;
    unsigned long long* const field = static_cast<unsigned long long*>(c->fg.mem);
    const uint32_t cur = c->fg.slot ^ 1u, prev = c->fg.slot;
    uint32_t* colors = reinterpret_cast<uint32_t*>(field + n_in);
    float* zs = reinterpret_cast<float*>(colors + 2 * n_out);
    FgBuffers b{};
    b.color = static_cast<const uint32_t*>(t->Color);
    b.depth = static_cast<const float*>(t->Depth);
    b.mv = static_cast<const float*>(t->MotionVector);
    b.out = static_cast<uint32_t*>(t->Output);
    b.prev_color = colors + prev * n_out;
    b.prev_z = zs + prev * n_in;
    b.hist_color = colors + cur * n_out;
    b.hist_z = zs + cur * n_in;
    b.field = field;
    if (generated) *generated = restart ? 0u : 1u;
    if (restart) {
        // step 0: Output = Color bit for bit, the current slot takes Color and Depth
        PT_HIP(c, hipMemcpyAsync(b.out, b.color, n_out * 4, hipMemcpyDeviceToDevice, c->stream));
        PT_HIP(c, hipMemcpyAsync(b.hist_color, b.color, n_out * 4, hipMemcpyDeviceToDevice, c->stream));
        PT_HIP(c, hipMemcpyAsync(b.hist_z, b.depth, n_in * 4, hipMemcpyDeviceToDevice, c->stream));
    } else {
        PT_HIP(c, hipMemsetAsync(b.field, 0xFF, n_in * 8, c->stream));
        PT_HIP(c, launch_framegen(b, fg_params(w, h, W, H, s->Format), c->stream));
    }
    history_commit(c->fg, s->Format);
    return PT_OK;
}

// Row N15 -- the ray-reconstruction stand-in (DESIGN.md spec S21): the prepare and the resolve launch on the context's stream, the
// history and the prepare pass's records in the context (kRrSlotBytesPerPixel, kRrRecordBytesPerPixel).
PtStatus pt_ray_reconstruction(PtContext* c, const PtRayReconstructionSettings* s, const PtRayReconstructionTextures* t)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!s || !t) return fail(c, PT_ERR_INVALID_ARG, "pt_ray_reconstruction: null pointer");
    const uint32_t w = s->RenderSize[0], h = s->RenderSize[1], W = s->OutputSize[0], H = s->OutputSize[1];
    if (w == 0 || h == 0 || w > kUpMaxSize || h > kUpMaxSize) return fail(c, PT_ERR_INVALID_ARG, "pt_ray_reconstruction: RenderSize must be in [1, 16384]");
    if (W < w || H < h || W > kUpMaxSize || H > kUpMaxSize || (uint64_t)W > (uint64_t)kUpMaxRatio * w || (uint64_t)H > (uint64_t)kUpMaxRatio * h)
        return fail(c, PT_ERR_INVALID_ARG, "pt_ray_reconstruction: OutputSize must be in [RenderSize, 4 * RenderSize] per axis and at most 16384");
    for (const float j : { s->Jitter[0], s->Jitter[1] })
        if (!is_finite(j) || !(pt_abs(j) <= 1.0f)) return fail(c, PT_ERR_INVALID_ARG, "pt_ray_reconstruction: Jitter must be finite and within [-1, 1]");
    float max_a = s->MaxHistoryWeight;
    if (max_a == 0.0f) max_a = kUpDefaultHistoryWeight;
    if (!is_finite(max_a) || !(max_a >= kUpMinHistoryWeight && max_a <= kUpMaxHistoryWeight))
        return fail(c, PT_ERR_INVALID_ARG, "pt_ray_reconstruction: MaxHistoryWeight must be 0 or in [1, 256]");
    for (const float v : s->Position)
        if (!is_finite(v)) return fail(c, PT_ERR_INVALID_ARG, "pt_ray_reconstruction: Position must be finite");
    for (int i = 0; i < 16; i++)
        if (!is_finite(s->ProjectionToView[i]) || !is_finite(s->ViewToWorld[i]) || !is_finite(s->PreviousWorldToProjection[i]))
            return fail(c, PT_ERR_INVALID_ARG, "pt_ray_reconstruction: every matrix entry must be finite");
    const uint64_t n_in = (uint64_t)w * h, n_out = (uint64_t)W * H;
    // the output must not share a byte with an input (a workgroup reads the inputs of its neighbours' pixels)
    const BufferUse use[8] = { {t->Color, n_in * 16, 16, false, true, "Color"}, {t->Depth, n_in * 4, 4, false, true, "Depth"},
                               {t->MotionVector, n_in * 12, 4, false, true, "MotionVector"}, {t->NormalRoughness, n_in * 16, 16, false, true, "NormalRoughness"},
                               {t->DiffuseAlbedo, n_in * 12, 4, false, true, "DiffuseAlbedo"}, {t->SpecularAlbedo, n_in * 12, 4, false, true, "SpecularAlbedo"},
                               {t->SpecularHitDistance, n_in * 4, 4, false, true, "SpecularHitDistance"}, {t->Output, n_out * 16, 16, true, true, "Output"} };
    if (const PtStatus st = buffers_ok(c, "pt_ray_reconstruction", use, 8); st != PT_OK) return st;
    PT_HIP(c, hipSetDevice(c->device));
    bool restart = s->Reset != 0 || !c->rr.valid;  // (a change of any size makes a new allocation, which restarts)
    if (const PtStatus st = history_begin(c, c->rr, {W, H, w, h}, 2 * n_out * kRrSlotBytesPerPixel + n_in * kRrRecordBytesPerPixel, restart); st != PT_OK) return st;
    // the allocation: hist[2], hist_n[2], the three records (float4 each), then hist_z[2] (float)
    float4* const f4 = static_cast<float4*>(c->rr.mem);
    float* const zs = reinterpret_cast<float*>(f4 + 4 * n_out + 3 * n_in);
    const uint32_t cur = c->rr.slot ^ 1u, prev = c->rr.slot;
    RrBuffers b{};
    b.color = static_cast<const float4*>(t->Color);
    b.depth = static_cast<const float*>(t->Depth);
    b.motion = static_cast<const float*>(t->MotionVector);
    b.normal_roughness = static_cast<const float4*>(t->NormalRoughness);
    b.diffuse_albedo = static_cast<const float*>(t->DiffuseAlbedo);
    b.specular_albedo = static_cast<const float*>(t->SpecularAlbedo);
    b.hit_distance = static_cast<const float*>(t->SpecularHitDistance);
    b.out = static_cast<float4*>(t->Output);
    b.prev_hist = f4 + prev * n_out;
    b.hist = f4 + cur * n_out;
    b.prev_n = f4 + (2 + prev) * n_out;
    b.hist_n = f4 + (2 + cur) * n_out;
    b.rec_tz = f4 + 4 * n_out;
    b.rec_nr = b.rec_tz + n_in;
    b.rec_virt = b.rec_nr + n_in;
    b.prev_z = zs + prev * n_out;
    b.hist_z = zs + cur * n_out;
    const RrParams R = rr_params(w, h, W, H, s->Jitter[0], s->Jitter[1], max_a, s->Position, s->ProjectionToView, s->ViewToWorld, s->PreviousWorldToProjection);
    PT_HIP(c, launch_ray_reconstruction(b, R, restart, c->stream));
    history_commit(c->rr, 0);
    return PT_OK;
}

PtStatus pt_ray_reconstruction_history(PtContext* c, void* history, void* normal, void* depth)
{
    if (!c) return PT_ERR_INVALID_ARG;
    if (!c->rr.valid || !c->rr.mem) return fail(c, PT_ERR_STATE, "pt_ray_reconstruction_history: no pt_ray_reconstruction call has been made");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t n_out = (uint64_t)c->rr.dims[0] * c->rr.dims[1], n_in = (uint64_t)c->rr.dims[2] * c->rr.dims[3];
    const float4* const f4 = static_cast<const float4*>(c->rr.mem);
    const float* const zs = reinterpret_cast<const float*>(f4 + 4 * n_out + 3 * n_in);
    if (history) PT_HIP(c, hipMemcpy(history, f4 + c->rr.slot * n_out, n_out * sizeof(float4), hipMemcpyDeviceToHost));
    if (normal) PT_HIP(c, hipMemcpy(normal, f4 + (2 + c->rr.slot) * n_out, n_out * sizeof(float4), hipMemcpyDeviceToHost));
    if (depth) PT_HIP(c, hipMemcpy(depth, zs + c->rr.slot * n_out, n_out * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
