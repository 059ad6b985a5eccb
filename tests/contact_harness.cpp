// Host build of exoplanet_amd/csrc/exo_contact.hpp for tests/test_contact_host.py: exo::contact_solve, the lines the
// kernels run, on rows of (a, e, cos w, sin w, cos i, sin i, L).  g++ -O2 -ffp-contract=off; a test harness, not a product
// path.  With CONTACT_HARNESS_MAIN: a stand-alone program over a dozen geometries (for a sanitizer build).
#define EXO_HOST_BUILD 1
#include <stdint.h>
#include <stdio.h>

#include "../exoplanet_amd/csrc/exo_contact.hpp"

extern "C" void contact_harness(const double* in, int64_t n, double* M_left, double* M_right, int32_t* flag) {
  for (int64_t i = 0; i < n; ++i) {
    const double* r = in + 7 * i;   // (sin i is not read: the solver forms 1 - cos^2 i, as the kernel does)
    flag[i] = exo::contact_solve(r[0], r[1], r[2], r[3], r[4], r[6], &M_left[i], &M_right[i]) ? 1 : 0;
  }
}

#ifdef CONTACT_HARNESS_MAIN
int main() {
  // a / R, e, omega, b / (1 + r), r: fast path, wide windows, S >= 0.98, grazing, misses, high e at the apsides and off them
  static const double geo[][5] = {{12, 0.3, 1.1, 0.36, 0.1},    {2.0, 0.01, 0.3, 0.0, 0.1},   {1.105, 0.0, 0.3, 0.0, 0.1},
                                  {50, 0.3, 1.1, 1 - 1e-8, 0.1}, {50, 0.3, 1.1, 1 + 1e-6, 0.1}, {3000, 0.999, 1.5707963267948966, 0.3, 0.1},
                                  {3000, 0.999, -1.5707963267948966, 0.3, 0.1}, {15, 0.9, 0.0, 0.2, 0.1}, {25, 0.9, 2.8415926535897933, 0.2, 0.1},
                                  {1.2, 0.1, 0.7, 0.1, 0.5},    {500, 0.2, 0.7, 0.2, 1.2},    {600, 0.995, 0.4, 0.0, 0.001}};
  int n_flag = 0;
  for (const auto& g : geo) {
    const double a = g[0], e = g[1], sw = sin(g[2]), cw = cos(g[2]), L = 1.0 + g[4];
    const double ci = (1.0 + e * sw) / ((1.0 - e) * (1.0 + e)) / a * (g[3] * L);
    const double in[7] = {a, e, cw, sw, ci, sqrt(fmax(0.0, 1.0 - ci * ci)), L};
    double ml, mr;
    int32_t flag;
    contact_harness(in, 1, &ml, &mr, &flag);
    n_flag += flag;
    printf("a=%g e=%g w=%g b=%.17g r=%g: flag %d  M_left %.17g  M_right %.17g\n", a, e, g[2], g[3] * L, g[4], flag, ml, mr);
    if (!flag && !(ml < mr)) return 1;
  }
  return n_flag == 2 ? 0 : 1;
}
#endif
