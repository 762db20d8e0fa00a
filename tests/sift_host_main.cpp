// The arithmetic of 3pre_amd/csrc/pre3_sift.h run by the host, stage after stage in the reference's own order: tests/test_sift_ref.py builds this
// with the host compiler and compares what it writes with tests/sift_ref.py.
//   sift_host_main <in.bin> <out.bin>      in: int32 M, N, strict; M * N doubles (column-major)
//   out: int32 O; per octave int32 M, N and its 6 Gaussian levels; int32 n_refined, then (x, y, s, octave) each; int32 K, then 4 doubles (0-based frame)
//   and 128 doubles (descriptor) each; int32 counts[4 * O]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pre3_sift.h"

using namespace pre3;

static void smooth(const SiftLevelPlan &lev, const double *src, double *dst, int M, int N)
{
    if (!(lev.sigma > 0.01)) { for (size_t i = 0; i < (size_t)M * N; ++i) dst[i] = src[i]; return; }
    std::vector<double> tmp((size_t)M * N);
    for (int c = 0; c < N; ++c) for (int r = 0; r < M; ++r) tmp[r + (size_t)c * M] = sift_tap_sum(lev.taps, lev.W, src + (size_t)c * M, 1, M, r);
    for (int c = 0; c < N; ++c) for (int r = 0; r < M; ++r) dst[r + (size_t)c * M] = sift_tap_sum(lev.taps, lev.W, tmp.data() + r, (size_t)M, N, c);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    int32_t hdr[3];
    if (fread(hdr, 4, 3, fi) != 3) return 2;
    const int M0 = hdr[0], N0 = hdr[1];
    const bool strict = hdr[2] != 0;
    std::vector<double> img((size_t)M0 * N0);
    if (fread(img.data(), 8, img.size(), fi) != img.size()) return 2;
    fclose(fi);
    SiftPlan plan;
    if (!sift_plan(M0, N0, &plan)) return 3;
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    int32_t O = plan.O;
    fwrite(&O, 4, 1, fo);
    std::vector<std::vector<double>> gss(O), dog(O);
    std::vector<double> cur((size_t)4 * M0 * N0);
    for (int c = 0; c < 2 * N0; ++c) for (int r = 0; r < 2 * M0; ++r) cur[r + (size_t)c * 2 * M0] = sift_double_size(img.data(), M0, N0, r, c, strict);
    for (int o = 0; o < O; ++o) {
        const int M = plan.rows[o], N = plan.cols[o];
        const size_t n = (size_t)M * N;
        if (o > 0) {
            cur.assign(n, 0.0);
            const int Mp = plan.rows[o - 1];
            const double *src = gss[o - 1].data() + (size_t)SIFT_SBEST_LEVEL * Mp * plan.cols[o - 1];
            for (int c = 0; c < N; ++c) for (int r = 0; r < M; ++r) cur[r + (size_t)c * M] = src[2 * r + (size_t)(2 * c) * Mp];
        }
        gss[o].resize(n * SIFT_NLEV); dog[o].resize(n * SIFT_NDOG);
        smooth(plan.lev[o ? 1 : 0][0], cur.data(), gss[o].data(), M, N);
        for (int l = 1; l < SIFT_NLEV; ++l) smooth(plan.lev[o ? 1 : 0][l], gss[o].data() + (l - 1) * n, gss[o].data() + l * n, M, N);
        for (size_t i = 0; i < n * SIFT_NDOG; ++i) dog[o][i] = gss[o][i + n] - gss[o][i];
        int32_t mn[2] = {M, N};
        fwrite(mn, 4, 2, fo);
        fwrite(gss[o].data(), 8, gss[o].size(), fo);
    }
    std::vector<double> cand, out;
    std::vector<int32_t> counts(4 * O, 0);
    for (int o = 0; o < O; ++o) {
        const int M = plan.rows[o], N = plan.cols[o];
        const double *D = dog[o].data();
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 1; s <= SIFT_NDOG - 2; ++s) for (int x = 1; x <= N - 2; ++x) for (int y = 1; y <= M - 2; ++y) {
                if (!sift_is_max(D, M, N, y, x, s, pass ? -1.0 : 1.0, 0.8 * SIFT_THRESH)) continue;
                ++counts[4 * o];
                if (!sift_inside(x, y, plan.pow2[s], plan.sigma0, M, N)) continue;
                ++counts[4 * o + 1];
                double q[3];
                if (!sift_refine(D, M, N, x, y, s, SIFT_THRESH, SIFT_R, q)) continue;
                ++counts[4 * o + 2];
                cand.insert(cand.end(), {q[0], q[1], q[2], (double)o});
            }
    }
    int32_t nc = (int32_t)(cand.size() / 4), K = 0;
    fwrite(&nc, 4, 1, fo);
    fwrite(cand.data(), 8, cand.size(), fo);
    for (int c = 0; c < nc; ++c) {
        const double *q = &cand[4 * c];
        const int o = (int)q[3], M = plan.rows[o], N = plan.cols[o];
        const SiftOrientSetup a = sift_orient_setup(q[0], q[1], q[2], plan.sigma0, M, N);
        if (!a.ok) continue;
        double H[SIFT_NBINS] = {0}, th[SIFT_MAX_PEAKS];
        const double *L = gss[o].data() + (size_t)a.si * M * N;
        for (int xs = (-a.W > 1 - a.xi ? -a.W : 1 - a.xi); xs <= (a.W < N - 2 - a.xi ? a.W : N - 2 - a.xi); ++xs)
            for (int ys = (-a.W > 1 - a.yi ? -a.W : 1 - a.yi); ys <= (a.W < M - 2 - a.yi ? a.W : M - 2 - a.yi); ++ys) {
                int bin; double amt;
                if (sift_orient_sample(L, M, a, xs, ys, &bin, &amt)) H[bin] += amt;
            }
        const int k = sift_orient_peaks(H, th);
        counts[4 * o + 3] += k;
        for (int j = 0; j < k; ++j) {
            double f[4];
            sift_frame(o, plan.sigma0, q[0], q[1], q[2], th[j], f);
            float d[128] = {0};
            const SiftDescSetup b = sift_desc_setup(q[0], q[1], q[2], th[j], plan.sigma0, M, N);
            if (b.ok) {
                const double *P = gss[o].data() + (size_t)b.si * M * N + b.yi + (size_t)b.xi * M;
                for (int dxi = (-b.W > 1 - b.xi ? -b.W : 1 - b.xi); dxi <= (b.W < N - 2 - b.xi ? b.W : N - 2 - b.xi); ++dxi)
                    for (int dyi = (-b.W > 1 - b.yi ? -b.W : 1 - b.yi); dyi <= (b.W < M - 2 - b.yi ? b.W : M - 2 - b.yi); ++dyi) {
                        float mod, angle, w[8]; int bins[8];
                        sift_gradient(P + (ptrdiff_t)dxi * M + dyi, M, &mod, &angle);
                        const int nb = sift_desc_sample(b, mod, angle, dxi, dyi, bins, w);
                        for (int i = 0; i < nb; ++i) d[bins[i]] += w[i];
                    }
                sift_desc_finish(d);
            }
            out.insert(out.end(), f, f + 4);
            for (int i = 0; i < 128; ++i) out.push_back((double)d[i]);
            ++K;
        }
    }
    fwrite(&K, 4, 1, fo);
    fwrite(out.data(), 8, out.size(), fo);
    fwrite(counts.data(), 4, counts.size(), fo);
    fclose(fo);
    return 0;
}
