// The host side of 3pre_amd/csrc/pre3_vocov.h (and pre3_predictu.h beside it): tests/test_vo_cov_ref.py builds this with the host compiler and compares
// what it writes with tests/vo_cov_ref.py.
//   vo_cov_host_main <in.bin> <out.bin>      in: int32 mode, then
//   mode 0 (the status rule): int32 n; n x int32 (sta, pnum, bad, dist_ok, status)
//          out: n x int32 (computes, predict takes, predict_u_select's take)
//   mode 1 (per-point terms): int32 n; n x (fp[3], fn[3], X[7]) doubles
//          out: n x (H_i full 7 x 7 row-major, B_i 7 x 6 row-major, r[3], C(fp)[9], C(fn)[9]) doubles
//   mode 2 (the whole covariance, on one thread): int32 pnum; pset1[3 * pnum], pset2[3 * pnum] (column-major), int32 inl[pnum], u[7]
//          out: int32 status, n_inliers; cov[49] (zeros unless status == 1)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pre3_predictu.h"
#include "pre3_vocov.h"

using namespace pre3;

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t mode = -1, n = 0;
    if (!rd(fi, &mode, 1) || !rd(fi, &n, 1) || n < 0) return 2;
    if (mode == 0) {
        for (int t = 0; t < n; ++t) {
            int32_t c[5];
            if (!rd(fi, c, 5)) return 2;
            const double uin[7] = { 1, 2, 3, 4, 5, 6, 7 };
            double uout[7];
            (void)predict_u_select(c[0], c[1], c[2], c[3], uin, uout);
            const int32_t o[3] = { vc_pair_computes(c[0], c[1], c[2], c[3]) ? 1 : 0, vc_predict_takes(c[0], c[1], c[2], c[3], c[4]) ? 1 : 0, uout[0] == 1.0 ? 1 : 0 };
            fwrite(o, 4, 3, fo);
        }
    } else if (mode == 1) {
        for (int t = 0; t < n; ++t) {
            double in[13], Hi[28], Bi[42], r[3], Cp[9], Cn[9], Hf[49];
            if (!rd(fi, in, 13)) return 2;
            vc_point_terms(in, in + 3, in + 6, Hi, Bi, r);
            vc_point_cov(in, Cp);
            vc_point_cov(in + 3, Cn);
            for (int a = 0; a < 7; ++a) for (int b = 0; b < 7; ++b) Hf[7 * a + b] = a >= b ? Hi[vc_ix(a, b)] : Hi[vc_ix(b, a)];
            fwrite(Hf, 8, 49, fo); fwrite(Bi, 8, 42, fo); fwrite(r, 8, 3, fo); fwrite(Cp, 8, 9, fo); fwrite(Cn, 8, 9, fo);
        }
    } else if (mode == 2) {
        const int pnum = n;
        std::vector<double> p1(3 * (size_t)pnum), p2(3 * (size_t)pnum);
        std::vector<int32_t> inl(pnum);
        double u[7], H[28] = { 0 }, M[28] = { 0 }, cov[49] = { 0 };
        if (!rd(fi, p1.data(), p1.size()) || !rd(fi, p2.data(), p2.size()) || !rd(fi, inl.data(), inl.size()) || !rd(fi, u, 7)) return 2;
        int32_t st[2] = { VC_NOT_COMPUTED, 0 };
        if (pnum >= 4) {
            bool finite = true;
            for (int k = 0; k < pnum; ++k)
                if (inl[k]) { ++st[1]; if (!vc_add_point(&p1[3 * (size_t)k], &p2[3 * (size_t)k], u, H, M)) finite = false; }
            st[0] = vc_finish(H, M, finite, cov);
        }
        fwrite(st, 4, 2, fo); fwrite(cov, 8, 49, fo);
    } else return 2;
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 2;
}
