// The dense ICP's loop-control rule (3pre_amd/csrc/pre3_icp.h: icp_ctl_start, icp_advance, icp_error) built for the host and stepped from standard input,
// for tests/test_icp_loop_host.py.  Built with -fsanitize=address,undefined; it links nothing of the library.
//   input:  res, then one "p sum_d" per line (sum_d as a C99 hexadecimal float)
//   output: per step "applied phase n c1 c2 no_change done status it1 it2 total p e1 e2 last_e" (doubles as hexadecimal floats), then "error <e>"
#include <cstdio>
#include <cstdlib>

#include "pre3_icp.h"

int main()
{
    char a[128], b[128];
    if (std::scanf("%127s", a) != 1) return 2;
    pre3::IcpCtl c;
    pre3::icp_ctl_start(&c, 0, 0, std::strtod(a, nullptr));
    while (std::scanf("%127s %127s", a, b) == 2) {
        const int p = std::atoi(a);
        const int applied = pre3::icp_advance(&c, p, std::strtod(b, nullptr));
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %a %a %a\n", applied, c.phase, c.n, c.c1, c.c2, c.no_change, c.done, c.status, c.it1, c.it2, c.total, c.p,
                    c.e1, c.e2, c.last_e);
    }
    std::printf("error %a\n", pre3::icp_error(&c));
    return 0;
}
