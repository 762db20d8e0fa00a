// pnp_host_main.cpp -- 3pre_amd/csrc/pre3_pnp.h (and pre3_svd3.h under it) run on the host: the text the kernels of pre3_pnp.hip run, with every sum
// over the points taken in index order.  tests/test_pnp_host.py builds it with the address and undefined-behaviour sanitizers and runs it as a
// program; tests/golden/make_pnp_tolerance.py measures with it what separates the Jacobi eigensolver from LAPACK (tests/epnp_ref.py).
//   pnp_host_main in out
//   in :  int32 ncases, then per case  int32 n, int32 pad, double f, Cx, Cy, Xw[n][3], U[n][2]
//   out:  per case  double R[9], T[3], u[7], err[3], best, sta, dim3, sweeps, w[12] (all eigenvalues, ascending), dist[n] (of the answer)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pre3_pnp.h"

using namespace pre3;

namespace {

struct Sol { double R[9], T[3], err; std::vector<double> dist; bool finite; };

void jacobi12(double *A, double *V, int *sweeps)
{
    double cs[12];
    int sw = 0;
    while (sw < PNP_SWEEPS && !pnp_jac_done(A)) {
        for (int r = 0; r < 11; ++r) {
            for (int k = 0; k < 6; ++k) pnp_jac_angle_item(A, r, k, cs);
            for (int it = 0; it < 72; ++it) pnp_jac_col_item(A, V, r, it, cs);
            for (int it = 0; it < 72; ++it) pnp_jac_row_item(A, r, it, cs);
        }
        ++sw;
    }
    *sweeps = sw;
}

Sol solve_dim(int n, const double *Xw, const double *U, double f, double Cx, double Cy, const double X[12])
{
    Sol s;
    double C[12], wc[3] = { 0, 0, 0 }, cc_[3] = { 0, 0, 0 };
    for (int i = 0; i < 12; ++i) C[i] = X[i];
    for (int k = 0; k < n; ++k) {
        double a[4], xc[3];
        pnp_alphas(Xw[3 * k], Xw[3 * k + 1], Xw[3 * k + 2], a);
        pnp_xc(a, C, xc);
        for (int t = 0; t < 3; ++t) { wc[t] += Xw[3 * k + t]; cc_[t] += xc[t]; }
    }
    for (int t = 0; t < 3; ++t) { wc[t] /= n; cc_[t] /= n; }
    double cc = 0, cw = 0;
    for (int k = 0; k < n; ++k) {
        double a[4], xc[3];
        pnp_alphas(Xw[3 * k], Xw[3 * k + 1], Xw[3 * k + 2], a);
        pnp_xc(a, C, xc);
        const double dc = pnp_dist3(xc, cc_), dw = pnp_dist3(Xw + 3 * k, wc);
        cc += dc * dc; cw += dc * dw;
    }
    pnp_scale(cc, cw, C);
    double sum[3] = { 0, 0, 0 };
    bool neg = false;
    for (int k = 0; k < n; ++k) {
        double a[4], xc[3];
        pnp_alphas(Xw[3 * k], Xw[3 * k + 1], Xw[3 * k + 2], a);
        pnp_xc(a, C, xc);
        for (int t = 0; t < 3; ++t) sum[t] += xc[t];
        neg = neg || xc[2] < 0;
    }
    const double sg = neg ? -1.0 : 1.0;
    double ccent[3], M[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int t = 0; t < 3; ++t) ccent[t] = sg * sum[t] / n;
    for (int k = 0; k < n; ++k) {
        double a[4], xc[3];
        pnp_alphas(Xw[3 * k], Xw[3 * k + 1], Xw[3 * k + 2], a);
        pnp_xc(a, C, xc);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M[3 * i + j] += (sg * xc[i] - ccent[i]) * (Xw[3 * k + j] - wc[j]);
    }
    pnp_getrot(M, ccent, wc, s.R, s.T);
    double P[12], e = 0;
    pnp_proj_matrix(s.R, s.T, f, Cx, Cy, P);
    s.dist.resize(n);
    for (int k = 0; k < n; ++k) { double zc; s.dist[k] = pnp_reproj(P, Xw + 3 * k, U[2 * k], U[2 * k + 1], &zc); e += s.dist[k]; }
    s.err = e / n;
    s.finite = pnp_finite(s.R, 9) && pnp_finite(s.T, 3) && pnp_finite(&s.err, 1);
    return s;
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
        int32_t hdr[2];
        double cam[3];
        if (fread(hdr, 4, 2, fi) != 2 || fread(cam, 8, 3, fi) != 3) return 3;
        const int n = hdr[0];
        if (n < PNP_MIN_N || n > PNP_MAX_N) return 4;
        std::vector<double> Xw(3 * (size_t)n), U(2 * (size_t)n);
        if (fread(Xw.data(), 8, Xw.size(), fi) != Xw.size() || fread(U.data(), 8, U.size(), fi) != U.size()) return 3;
        const double f = cam[0], Cx = cam[1], Cy = cam[2];
        double acc[PNP_MTM], A[144], V[144], w6[42];
        for (int i = 0; i < PNP_MTM; ++i) acc[i] = 0;
        for (int k = 0; k < n; ++k) {
            double a[4];
            pnp_alphas(Xw[3 * k], Xw[3 * k + 1], Xw[3 * k + 2], a);
            pnp_mtm_point(a, f, Cx - U[2 * k], Cy - U[2 * k + 1], acc);
        }
        for (int e = 0; e < 144; ++e) pnp_mtm_entry(acc, e, A, V);
        double out[9 + 3 + 7 + 3 + 4 + 12];
        for (double &v : out) v = NAN;
        std::vector<double> dist(n, NAN);
        int32_t best = 0, sta = PNP_NONFINITE;
        int sweeps = 0, dim3 = 0;
        double err[3] = { NAN, NAN, NAN };
        Sol sol[3];
        if (pnp_finite(acc, PNP_MTM)) {
            jacobi12(A, V, &sweeps);
            int32_t ord[3];
            pnp_order3(A, ord);
            for (int t = 0; t < 3; ++t) pnp_fix_sign(V, ord[t]);
            double X[12];
            for (int i = 0; i < 12; ++i) X[i] = V[12 * i + ord[0]];
            sol[0] = solve_dim(n, Xw.data(), U.data(), f, Cx, Cy, X);
            pnp_dim2(V, ord, X);
            sol[1] = solve_dim(n, Xw.data(), U.data(), f, Cx, Cy, X);
            err[0] = sol[0].err; err[1] = sol[1].err;
            bool finite = sol[0].finite && sol[1].finite;
            int nd = 2;
            if (finite && pnp_enters_dim3(err[0], err[1])) {
                dim3 = 1; nd = 3;
                pnp_dim3(V, ord, w6, X);
                sol[2] = solve_dim(n, Xw.data(), U.data(), f, Cx, Cy, X);
                err[2] = sol[2].err;
                finite = finite && sol[2].finite;
            }
            pnp_answer(err, nd, finite, &best, &sta);
            double w[12];
            for (int i = 0; i < 12; ++i) w[i] = A[13 * i];
            std::sort(w, w + 12);
            memcpy(out + 26, w, sizeof w);
            if (sta != PNP_NONFINITE) {
                memcpy(out, sol[best].R, 72); memcpy(out + 9, sol[best].T, 24);
                pnp_pair_u(sol[best].R, sol[best].T, out + 12);
                dist = sol[best].dist;
            }
        }
        out[19] = err[0]; out[20] = err[1]; out[21] = err[2];
        out[22] = best; out[23] = sta; out[24] = dim3; out[25] = sweeps;
        if (fwrite(out, 8, sizeof out / 8, fo) != sizeof out / 8 || fwrite(dist.data(), 8, dist.size(), fo) != dist.size()) return 5;
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 5;
}
