// The host side of 3pre_amd/csrc/pre3_predicticp.h and pre3_icpcov.h (over pre3_vocov.h): tests/test_icp_cov_ref.py builds this with the host compiler
// (-fsanitize=address,undefined where the compiler has them) and compares what it writes with tests/icp_cov_ref.py.
//   icp_cov_host_main <in.bin> <out.bin>      in: int32 mode, int32 n, then
//   mode 0 (the selection rule): n x { int32 sta, pnum, bad, dist_ok, icp_sta, icp_u_finite, noise, cov_pair_status, cov_icp_status, pad; double error, max_error }
//          out: n x int32 (refusal, u_taken, noise_taken, which u came out: 0 identity, 1 the pair's, 2 the ICP's)
//   mode 1 (the tree of partial sums, restated on one thread): n = p; p x (fp[3], fn[3]) doubles; u[7]
//          out: int32 status, n; cov[49] (zeros unless status == 1)
// Mode 1 is k_icp_cov_part / k_icp_cov_fin's order of additions: one pair per thread into zeroed sums, the 64 lanes of a wave joined by the xor butterfly,
// the four waves in wave order; then thread t of the finisher takes partials t, t + 256, ... ascending, and the same join.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pre3_icpcov.h"
#include "pre3_predicticp.h"

using namespace pre3;

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

struct Sums { std::array<double, 56> v; int n, nonfinite; };

// 256 threads' sums joined as both kernels join them
static Sums block_join(std::vector<Sums> t)
{
    const int NW = IC_PAIRS / 64;
    for (int w = 0; w < NW; ++w)
        for (int o = 32; o > 0; o >>= 1) {
            std::vector<Sums> old(t.begin() + 64 * w, t.begin() + 64 * (w + 1));
            for (int l = 0; l < 64; ++l) {
                Sums &d = t[64 * w + l];
                for (int i = 0; i < 56; ++i) d.v[i] = old[l].v[i] + old[l ^ o].v[i];
                d.n = old[l].n + old[l ^ o].n; d.nonfinite = old[l].nonfinite | old[l ^ o].nonfinite;
            }
        }
    Sums s = t[0];
    for (int w = 1; w < NW; ++w) {
        for (int i = 0; i < 56; ++i) s.v[i] = s.v[i] + t[64 * w].v[i];
        s.n += t[64 * w].n; s.nonfinite |= t[64 * w].nonfinite;
    }
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t mode = -1, n = 0;
    if (!rd(fi, &mode, 1) || !rd(fi, &n, 1) || n < 0) return 2;
    if (mode == 0) {
        for (int t = 0; t < n; ++t) {
            int32_t c[10];
            double e[2];
            if (!rd(fi, c, 10) || !rd(fi, e, 2)) return 2;
            const double u_pair[7] = { 1, 2, 3, 4, 5, 6, 7 };
            double u_icp[7] = { 11, 12, 13, 14, 15, 16, 17 }, u_out[7];
            if (!c[5]) u_icp[t % 7] = (t & 1) ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
            int ut = -1, nt = -1;
            const int refusal = predict_icp_select(c[0], c[1], c[2], c[3], u_pair, c[4], u_icp, e[0], e[1], c[6], c[7], c[8], u_out, &ut, &nt);
            bool is_icp = true, is_pair = true, is_id = true;
            for (int i = 0; i < 7; ++i) {
                is_icp = is_icp && u_out[i] == u_icp[i]; is_pair = is_pair && u_out[i] == u_pair[i]; is_id = is_id && u_out[i] == (i == 3 ? 1.0 : 0.0);
            }
            const int32_t o[4] = { refusal, ut, nt, is_icp ? 2 : is_pair ? 1 : is_id ? 0 : -1 };
            fwrite(o, 4, 4, fo);
        }
    } else if (mode == 1) {
        const int p = n;
        std::vector<double> pts(6 * (size_t)p);
        double u[7], cov[49] = { 0 };
        if (!rd(fi, pts.data(), pts.size()) || !rd(fi, u, 7)) return 2;
        int32_t st[2] = { VC_NOT_COMPUTED, 0 };
        if (ic_computes(1, p, IC_MAX_P)) {
            const int nparts = ic_parts(p);
            std::vector<Sums> part(nparts);
            for (int w = 0; w < nparts; ++w) {
                std::vector<Sums> th(IC_PAIRS);
                for (int t = 0; t < IC_PAIRS; ++t) {
                    Sums &s = th[t];
                    s.v.fill(0.0); s.n = 0; s.nonfinite = 0;
                    const int k = IC_PAIRS * w + t;
                    if (k < p) { s.n = 1; if (!vc_add_point(&pts[6 * (size_t)k], &pts[6 * (size_t)k + 3], u, s.v.data(), s.v.data() + 28)) s.nonfinite = 1; }
                }
                part[w] = block_join(th);
            }
            std::vector<Sums> th(IC_FIN_THREADS);
            for (int t = 0; t < IC_FIN_THREADS; ++t) {
                Sums &s = th[t];
                s.v.fill(0.0); s.n = 0; s.nonfinite = 0;
                for (int q = t; q < nparts; q += IC_FIN_THREADS) {
                    for (int i = 0; i < 56; ++i) s.v[i] = s.v[i] + part[q].v[i];
                    s.n += part[q].n; s.nonfinite |= part[q].nonfinite;
                }
            }
            const Sums tot = block_join(th);
            st[1] = tot.n;
            st[0] = vc_finish(tot.v.data(), tot.v.data() + 28, tot.nonfinite == 0, cov);
        }
        fwrite(st, 4, 2, fo); fwrite(cov, 8, 49, fo);
    } else return 2;
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 2;
}
