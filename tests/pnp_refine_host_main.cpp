// pnp_refine_host_main.cpp -- 3pre_amd/csrc/pre3_pnpref.h and reloc_noise_from_pose of pre3_reloc.h run on the host: the text k_pnp_refine
// (pre3_pnp.hip) and k_predict's PnRelocRef form (pre3_geom.hip) run, with every sum over the points taken in index order.
// tests/test_pnp_refine_host.py builds it with the address and undefined-behaviour sanitizers and runs it as a program;
// tests/golden/make_pnp_refine_tolerance.py measures with it what separates this text from tests/pnp_refine_ref.py.
//   pnp_refine_host_main in out
//   in :  int32 ncases, then per case  int32 n, n_iter, sta_in, pad, double f, Cx, Cy, sigma_px, R0[9], T0[3], x7[7], Xw[n][3], U[n][2]
//   out:  per case  double R[9], T[3], u[7], cost[11], cov6[36], cov7[49], sigma2, sta, Pn[49] (reloc_noise_from_pose(x7, cov7); NaN unless sta is 1 or 2)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pre3_pnpref.h"
#include "pre3_reloc.h"

using namespace pre3;

namespace {

constexpr int REC = 9 + 3 + 7 + 11 + 36 + 49 + 1 + 1 + 49;

bool pass(int n, const double *Xw, const double *U, double f, double Cx, double Cy, const double R[9], const double T[3], double acc[PNPREF_SUMS])
{
    bool front = true;
    for (int i = 0; i < PNPREF_SUMS; ++i) acc[i] = 0;
    for (int k = 0; k < n; ++k) front = (pnpref_point(R, T, f, Cx, Cy, Xw + 3 * k, U[2 * k], U[2 * k + 1], acc) > 0) && front;
    return front;
}

// k_pnp_refine's body, statement for statement
void refine(int n, int n_iter, int sta_in, double f, double Cx, double Cy, double sigma_px, const double R0[9], const double T0[3], const double x7[7], const double *Xw,
            const double *U, double out[REC])
{
    for (int i = 0; i < REC; ++i) out[i] = NAN;
    double *oR = out, *oT = out + 9, *ou = out + 12, *ocost = out + 19, *ocov6 = out + 30, *ocov7 = out + 66, *os2 = out + 115, *osta = out + 116, *oPn = out + 117;
    memcpy(oR, R0, 72); memcpy(oT, T0, 24);
    pnp_pair_u(R0, T0, ou);
    *osta = PNPREF_NOT_COMPUTED;
    if (!(sta_in == PNP_OK || sta_in == PNP_BEST_OF_THREE) || n < PNP_MIN_N) return;
    double R[9], T[3], acc[PNPREF_SUMS], cost_first = 0;
    memcpy(R, R0, 72); memcpy(T, T0, 24);
    bool fin = true;
    for (int k = 0; k < n_iter; ++k) {
        (void)pass(n, Xw, U, f, Cx, Cy, R, T, acc);
        if (k == 0) cost_first = acc[27];
        ocost[k] = acc[27];
        fin = fin && pnp_finite(acc, PNPREF_SUMS);
        fin = pnpref_step(acc, R, T) && fin;
        fin = fin && pnp_finite(R, 9) && pnp_finite(T, 3);
    }
    bool front = pass(n, Xw, U, f, Cx, Cy, R, T, acc);
    if (n_iter == 0) cost_first = acc[27];
    ocost[n_iter] = acc[27];
    fin = fin && pnp_finite(acc, PNPREF_SUMS);
    const bool taken = pnpref_takes(n_iter, fin, front, cost_first, acc[27]);
    if (!taken && n_iter >= 1) {
        memcpy(R, R0, 72); memcpy(T, T0, 24);
        front = pass(n, Xw, U, f, Cx, Cy, R, T, acc);
    }
    double u[7], cov6[36], cov7[49];
    const double s2 = pnpref_sigma2(sigma_px, acc[27], n);
    pnp_pair_u(R, T, u);
    bool ok = front && pnp_finite(acc, PNPREF_SUMS) && isfinite(s2) && pnp_finite(u, 7);
    ok = ok && pnpref_cov6(acc, s2, cov6);
    ok = ok && pnpref_cov7(R, u, cov6, cov7);
    if (!ok) { *osta = PNPREF_NO_COV; return; }
    memcpy(oR, R, 72); memcpy(oT, T, 24); memcpy(ou, u, 56); memcpy(ocov6, cov6, sizeof cov6); memcpy(ocov7, cov7, sizeof cov7);
    *os2 = s2; *osta = taken ? PNPREF_TAKEN : PNPREF_KEPT;
    reloc_noise_from_pose(x7, cov7, oPn);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, fi) != 1) return 3;
    for (int cs = 0; cs < ncases; ++cs) {
        int32_t hdr[4];
        double p[4 + 9 + 3 + 7];
        if (fread(hdr, 4, 4, fi) != 4 || fread(p, 8, 23, fi) != 23) return 3;
        const int n = hdr[0];
        if (n < 0 || n > PNP_MAX_N || hdr[1] < 0 || hdr[1] > PNPREF_MAX_ITER) return 4;
        std::vector<double> Xw(3 * (size_t)n + 1), U(2 * (size_t)n + 1);
        if (fread(Xw.data(), 8, 3 * (size_t)n, fi) != 3 * (size_t)n || fread(U.data(), 8, 2 * (size_t)n, fi) != 2 * (size_t)n) return 3;
        double out[REC];
        refine(n, hdr[1], hdr[2], p[0], p[1], p[2], p[3], p + 4, p + 13, p + 16, Xw.data(), U.data(), out);
        if (fwrite(out, 8, REC, fo) != (size_t)REC) return 5;
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 5;
}
