// Host build of csrc/preview_reg.hpp for tests/test_preview_reg_cpu.py and tests/test_gpu_preview_reg.py:
//   g++ -O2 -ffp-contract=off -shared -fPIC preview_reg.cpp -o _preview_reg.so
// One point after the other, one entry after the other, every rule taken from the header (the kernel spreads the same calls over
// threads that own 4 entries each).
#include "../../mipnerf_pl_amd/csrc/preview_reg.hpp"

extern "C" {

void hm_preview_reg_grad(int nx, int ny, int nz, int degree, const float* scale, const float* master, const unsigned char* mask, float* grad,
                         float w_sigma, float w_colour, float w_view, float eps) {
    const mip::PreviewReg p = {nx, ny, nz, {scale[0], scale[1], scale[2]}, w_sigma, w_colour, w_view, eps};
    const int W = mip::preview_row_halves(degree), used = mip::reg_row_used(degree);
    const long long step[3] = {1, nx, (long long)nx * ny};
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                if (!mip::reg_present(p, mask, x, y, z)) continue;
                const long long at = ((long long)z * ny + y) * nx + x;
                mip::RegStencil s;
                mip::reg_stencil(p, mask, x, y, z, &s);
                for (int e = 0; e < used; ++e) {
                    if (!mip::reg_touches(p, e)) continue;
                    float fwd[3], back[3], side[3][3];
                    for (int a = 0; a < 3; ++a) {
                        fwd[a] = s.fwd[a] ? master[(at + step[a]) * W + e] : 0.0f;
                        back[a] = s.back[a] ? master[(at - step[a]) * W + e] : 0.0f;
                        for (int b = 0; b < 3; ++b) side[a][b] = b != a && s.side[a][b] ? master[(at - step[a] + step[b]) * W + e] : 0.0f;
                    }
                    grad[at * W + e] = mip::reg_add(p, s, e, grad[at * W + e], master[at * W + e], fwd, back, side);
                }
            }
}

}  // extern "C"
