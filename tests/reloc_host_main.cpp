// reloc_host_main.cpp -- 3pre_amd/csrc/pre3_reloc.h run on the host: the rule lane 0 of every block of k_predict evaluates behind
// pre3_relocalise_seeded's RANSAC.  tests/test_reloc_host.py builds it with the address and undefined-behaviour sanitizers and
// runs it as a program against tests/reloc_ref.py; tests/golden/make_reloc_tolerance.py measures with it.
//   reloc_host_main in out
//   in :  int32 ncases, int32 pad, then per case  double x[7], pnp_u[7], int32 sta, n_support, min_support, pad
//   out:  per case  double u[7], taken, takes (reloc_takes alone), pose[7] (the prediction's r + R(q) u_r and q (x) u_q, normalised)
#include <cstdint>
#include <cstdio>

#include "pre3_reloc.h"

using namespace pre3;

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t hdr[2];
    if (fread(hdr, 4, 2, fi) != 2) return 3;
    for (int cs = 0; cs < hdr[0]; ++cs) {
        double in[14], out[16];
        int32_t w[4];
        if (fread(in, 8, 14, fi) != 14 || fread(w, 4, 4, fi) != 4) return 3;
        const double *x = in, *pnp_u = in + 7;
        out[7] = reloc_select(x, w[0], w[1], w[2], pnp_u, out);
        out[8] = reloc_takes(w[0], w[1], w[2]) ? 1.0 : 0.0;
        // predict_state_and_covariance.m:60-77 on the pose (pre3_geomdev.h: predict_pose), with the rule's own q2R
        double R[9], q[4];
        reloc_q2R(x + 3, R);
        const double a = x[3], b = x[4], c = x[5], d = x[6], ww = out[3], xx = out[4], y = out[5], z = out[6];
        q[0] = a * ww - b * xx - c * y - d * z; q[1] = a * xx + b * ww + c * z - d * y; q[2] = a * y - b * z + c * ww + d * xx; q[3] = a * z + b * y - c * xx + d * ww;
        const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int i = 0; i < 3; ++i) out[9 + i] = x[i] + (R[3 * i] * out[0] + R[3 * i + 1] * out[1] + R[3 * i + 2] * out[2]);
        for (int i = 0; i < 4; ++i) out[12 + i] = q[i] / nq;
        if (fwrite(out, 8, 16, fo) != 16) return 5;
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 5;
}
