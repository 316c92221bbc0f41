// rr_host.cpp -- TEST SHIM: compiles the product's ray-reconstruction header (csrc/pt_rr.h) as plain host C++ (the flags of
// upscale_host.cpp) so the tests can check it against the numpy restatement without a GPU, and the GPU kernels against it bit for
// bit.  Not part of the product; never loaded by it.
#include <vector>

#include "../../directx-raytracing-spheres-demo_amd/csrc/pt_rr.h"

using namespace pt;

namespace {

// size = {w, h, W, H}; fprm = {Jitter.x, Jitter.y, MaxHistoryWeight (not 0), Position[3], ProjectionToView[16], ViewToWorld[16],
// PreviousWorldToProjection[16]}
RrParams params_of(const uint32_t* size, const float* fprm)
{
    return rr_params(size[0], size[1], size[2], size[3], fprm[0], fprm[1], fprm[2], fprm + 3, fprm + 6, fprm + 22, fprm + 38);
}

// ptrs = Color, Depth, MotionVector, NormalRoughness, DiffuseAlbedo, SpecularAlbedo, SpecularHitDistance, Output, rec_tz, rec_nr,
// rec_virt, prev_hist, prev_n, prev_z, hist, hist_n, hist_z (the previous slot may be null on a restart)
RrBuffers buffers_of(void* const* ptrs)
{
    RrBuffers b{};
    b.color = static_cast<const float4*>(ptrs[0]);
    b.depth = static_cast<const float*>(ptrs[1]);
    b.motion = static_cast<const float*>(ptrs[2]);
    b.normal_roughness = static_cast<const float4*>(ptrs[3]);
    b.diffuse_albedo = static_cast<const float*>(ptrs[4]);
    b.specular_albedo = static_cast<const float*>(ptrs[5]);
    b.hit_distance = static_cast<const float*>(ptrs[6]);
    b.out = static_cast<float4*>(ptrs[7]);
    b.rec_tz = static_cast<float4*>(ptrs[8]);
    b.rec_nr = static_cast<float4*>(ptrs[9]);
    b.rec_virt = static_cast<float4*>(ptrs[10]);
    b.prev_hist = static_cast<const float4*>(ptrs[11]);
    b.prev_n = static_cast<const float4*>(ptrs[12]);
    b.prev_z = static_cast<const float*>(ptrs[13]);
    b.hist = static_cast<float4*>(ptrs[14]);
    b.hist_n = static_cast<float4*>(ptrs[15]);
    b.hist_z = static_cast<float*>(ptrs[16]);
    return b;
}

void prepare(const RrParams& R, const RrBuffers& b)
{
    for (int y = 0; y < (int)R.up.h; y++)  // what each lane of rr_prepare_kernel does
        for (int x = 0; x < (int)R.up.w; x++) {
            const RrRecord rec = rr_prepare_px(R, b, x, y);
            const size_t i = (size_t)y * R.up.w + x;
            b.rec_tz[i] = rec.tz;
            b.rec_nr[i] = rec.nr;
            b.rec_virt[i] = rec.virt;
        }
}

}  // namespace

extern "C" {

// the prepare pass alone: fills rec_tz, rec_nr, rec_virt
void rr_host_prepare(const uint32_t* size, const float* fprm, void* const* ptrs)
{
    prepare(params_of(size, fprm), buffers_of(ptrs));
}

// One call of pt_ray_reconstruction.  tiled = 0: the resolve pass reads the whole image's records; tiled = 1: the way pt_rr.hip runs
// it, per 32 x 8 block of output pixels a tile of kRrTileW x kRrTileH records staged over rr_footprint.  Returns the number of blocks
// whose lanes' taps do not fit the staged footprint (0 = the kernel's LDS tile holds every tap).
uint32_t rr_host_frame(const uint32_t* size, const float* fprm, uint32_t restart, uint32_t tiled, void* const* ptrs)
{
    const RrParams R = params_of(size, fprm);
    const UpParams& P = R.up;
    const RrBuffers b = buffers_of(ptrs);
    prepare(R, b);
    const size_t n = (size_t)P.w * P.h;
    if (!tiled) {
        std::vector<float> v[3] = { std::vector<float>(n), std::vector<float>(n), std::vector<float>(n) };
        for (size_t i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) v[k][i] = b.motion[3 * i + k];
        RrTile T;
        T.tz = b.rec_tz; T.nr = b.rec_nr; T.vx = v[0].data(); T.vy = v[1].data(); T.vz = v[2].data();
        T.x0 = 0; T.y0 = 0; T.stride = (int)P.w;
        for (int y = 0; y < (int)P.H; y++)
            for (int x = 0; x < (int)P.W; x++) {
                if (restart) rr_pixel<true>(R, T, b, x, y);
                else rr_pixel<false>(R, T, b, x, y);
            }
        return 0;
    }
    uint32_t misfits = 0;
    const int cells = kRrTileW * kRrTileH;
    std::vector<float4> tz(cells), nr(cells);
    std::vector<float> v[3] = { std::vector<float>(cells), std::vector<float>(cells), std::vector<float>(cells) };
    for (int Y0 = 0; Y0 < (int)P.H; Y0 += kUpBlockH)
        for (int X0 = 0; X0 < (int)P.W; X0 += kUpBlockW) {
            const UpFootprint F = rr_footprint(P, X0, Y0);
            bool fits = true;
            for (int ly = 0; ly < F.fh; ly++)
                for (int lx = 0; lx < F.fw; lx++) {
                    const size_t g = (size_t)(F.y0 + ly) * P.w + (F.x0 + lx);
                    const int s = ly * kRrTileW + lx;
                    tz[s] = b.rec_tz[g];
                    nr[s] = b.rec_nr[g];
                    for (int k = 0; k < 3; k++) v[k][s] = b.motion[3 * g + k];
                }
            RrTile T;
            T.tz = tz.data(); T.nr = nr.data(); T.vx = v[0].data(); T.vy = v[1].data(); T.vz = v[2].data();
            T.x0 = F.x0; T.y0 = F.y0; T.stride = kRrTileW;
            for (int y = Y0; y < Y0 + kUpBlockH && y < (int)P.H; y++)
                for (int x = X0; x < X0 + kUpBlockW && x < (int)P.W; x++) {
                    // every tap of the lane inside the image must be inside the staged footprint
                    const int nx = up_nearest((float)x + 0.5f, P.rx, P.w), ny = up_nearest((float)y + 0.5f, P.ry, P.h);
                    const int lo_x = nx - 2 < 0 ? 0 : nx - 2, hi_x = nx + 2 > (int)P.w - 1 ? (int)P.w - 1 : nx + 2;
                    const int lo_y = ny - 2 < 0 ? 0 : ny - 2, hi_y = ny + 2 > (int)P.h - 1 ? (int)P.h - 1 : ny + 2;
                    if (lo_x < F.x0 || hi_x >= F.x0 + F.fw || lo_y < F.y0 || hi_y >= F.y0 + F.fh) { fits = false; continue; }
                    if (restart) rr_pixel<true>(R, T, b, x, y);
                    else rr_pixel<false>(R, T, b, x, y);
                }
            if (!fits) misfits++;
        }
    return misfits;
}

// The widest footprint (rr_footprint_extent, before the tile bounds it) of any block along one axis with n_in input and n_out
// output pixels; block = 32 gives the columns, block = 8 the rows (the two axes run the same arithmetic).
uint32_t rr_host_max_extent(uint32_t n_in, uint32_t n_out, uint32_t block)
{
    const UpParams P = block == (uint32_t)kUpBlockW ? up_params(n_in, 1, n_out, 1, 0.0f, 0.0f, 1.0f) : up_params(1, n_in, 1, n_out, 0.0f, 0.0f, 1.0f);
    int widest = 0;
    for (int O0 = 0; O0 < (int)n_out; O0 += (int)block) {
        const UpFootprint F = block == (uint32_t)kUpBlockW ? rr_footprint_extent(P, O0, 0) : rr_footprint_extent(P, 0, O0);
        const int e = block == (uint32_t)kUpBlockW ? F.fw : F.fh;
        widest = e > widest ? e : widest;
    }
    return (uint32_t)widest;
}

uint32_t rr_host_tile_w() { return kRrTileW; }
uint32_t rr_host_tile_h() { return kRrTileH; }

}  // extern "C"
