// Stand-alone CPU program over csrc/camera_models.hpp (TEST INFRASTRUCTURE; tests/test_camera_models_cpu.py builds it with
// -fsanitize=address,undefined and runs it).  Input file, written by the test from the float64 restatement:
//     <number of parameter sets>
//     <mode> <k0> <k1> <k2> <k3> <n>            per set, followed by n lines
//     <xd> <yd> <c0> <c1> <c2>                  distorted normalised point and the restatement's camera direction
// Every point is undistorted in double and in float through the header; the program prints the largest absolute error of each and
// exits 1 when the double one exceeds <tol64> or the float one <tol32> (argv[2], argv[3]), 2 on a malformed file.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mipnerf_pl_amd/csrc/camera_models.hpp"

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <points file> <tol64> <tol32>\n", argv[0]);
        return 2;
    }
    const double tol64 = std::atof(argv[2]), tol32 = std::atof(argv[3]);
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int sets = 0;
    if (std::fscanf(f, "%d", &sets) != 1) return 2;
    int bad = 0;
    for (int s = 0; s < sets; ++s) {
        int mode = 0, n = 0;
        double k[4];
        if (std::fscanf(f, "%d %lf %lf %lf %lf %d", &mode, &k[0], &k[1], &k[2], &k[3], &n) != 6 || n < 0 || (mode != 2 && mode != 3)) return 2;
        std::vector<double> rows((size_t)n * 5);
        for (size_t i = 0; i < rows.size(); ++i)
            if (std::fscanf(f, "%lf", &rows[i]) != 1) return 2;
        const float kf[4] = {(float)k[0], (float)k[1], (float)k[2], (float)k[3]};
        double e64 = 0.0, e32 = 0.0;
        for (int i = 0; i < n; ++i) {
            const double* r = &rows[(size_t)i * 5];
            double c[3];
            float cf[3];
            camera_models::undistorted_direction<double>(mode, k, r[0], r[1], c);
            camera_models::undistorted_direction<float>(mode, kf, (float)r[0], (float)r[1], cf);
            for (int j = 0; j < 3; ++j) {
                e64 = std::fmax(e64, std::fabs(c[j] - r[2 + j]));
                e32 = std::fmax(e32, std::fabs((double)cf[j] - r[2 + j]));
            }
        }
        std::printf("set %d mode %d: max |double - restatement| = %.3e, max |float - restatement| = %.3e\n", s, mode, e64, e32);
        if (!(e64 <= tol64) || !(e32 <= tol32)) ++bad;
    }
    std::fclose(f);
    // degenerate inputs stay finite: a vanishing determinant is a zero step, a diverged solve falls back to the distorted point
    const double kd[4] = {-0.9, 0.0, 0.0, 0.0};
    double c[3];
    camera_models::undistorted_direction<double>(2, kd, 0.98, 0.7, c);
    if (!std::isfinite(c[0]) || !std::isfinite(c[1])) ++bad;
    const double kz[4] = {0.0, 0.0, 0.0, 0.0};
    camera_models::undistorted_direction<double>(2, kz, 0.3, -0.2, c);
    if (c[0] != 0.3 || c[1] != 0.2 || c[2] != -1.0) ++bad;                 // zero coefficients: exactly the pinhole direction
    camera_models::undistorted_direction<double>(3, kz, 0.0, 0.0, c);
    if (c[0] != 0.0 || c[1] != 0.0 || c[2] != -1.0) ++bad;                 // the fisheye's centre pixel
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
