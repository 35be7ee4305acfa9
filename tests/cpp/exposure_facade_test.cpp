// The exposure / attainment call of the C++ host facade (include/pharmsol_hip.hpp): Resident::exposure_attainment on a
// small two-compartment population, device 0.  Prints, per profile, the probability of target attainment and the
// weighted mean of the AUC as hex floats; tests/test_cpp_exposure.py runs the same design through the Python path and
// compares the bits.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../include/pharmsol_hip.hpp"

using namespace pharmsol;
using equation::Analytical;
using equation::Route;

int main() {
  Analytical m(PMX_K_TWO_COMPARTMENTS, 4);
  m.with_nstates(2).with_ndrugs(1).with_nout(1).with_output(0, 0, 3);
  m.with_metadata({"ke", "kcp", "kpc", "v"}, {"cp"}, {Route::infusion("iv", 0)});
  Data data;
  for (int s = 0; s < 5; ++s) {
    auto b = Subject::builder(std::to_string(s)).infusion(0.0, 500.0 + 25.0 * s, "iv", 0.5);
    for (double t : {0.5, 1.0, 2.0, 4.0, 8.0, 12.0, 24.0}) b.observation(t, 0.0, "cp");
    data.push_back(b.build());
  }
  const int P = 8;
  std::vector<double> theta, w(P, 0.125);
  for (int p = 0; p < P; ++p) {
    theta.push_back(0.05 + 0.03125 * p);
    theta.push_back(0.125 + 0.015625 * p);
    theta.push_back(0.0625 + 0.0078125 * p);
    theta.push_back(20.0 + 2.0 * p);
  }
  try {
    equation::Equation::Resident pop(m, data);
    const int64_t n = pop.n_profiles();
    if (n != 5) {
      std::printf("FAIL n_profiles %lld\n", static_cast<long long>(n));
      return 1;
    }
    std::vector<double> target(n, 60.0), pta(n, -7.0), mean(n, -7.0);
    std::vector<uint8_t> status(5 * P, 9);
    const double inf = std::numeric_limits<double>::infinity();
    pop.exposure_attainment(theta.data(), P, w.data(), nullptr, PMX_AUC_LINEAR, -inf, inf, 0.0, PMX_EXPO_AUC, target.data(),
                            pta.data(), mean.data(), status.data(), true);
    for (uint8_t s : status)
      if (s != 0) {
        std::printf("FAIL status %d\n", s);
        return 1;
      }
    for (int64_t k = 0; k < n; ++k) std::printf("profile %lld pta %a mean %a\n", static_cast<long long>(k), pta[k], mean[k]);
    // a refusal comes back as an exception: two metric bits
    bool threw = false;
    try {
      pop.exposure_attainment(theta.data(), P, w.data(), nullptr, PMX_AUC_LINEAR, -inf, inf, 0.0, PMX_EXPO_AUC | PMX_EXPO_CMAX,
                              target.data(), pta.data(), mean.data(), nullptr);
    } catch (const std::exception&) {
      threw = true;
    }
    if (!threw) {
      std::printf("FAIL two metric bits were accepted\n");
      return 1;
    }
  } catch (const std::exception& e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
  std::printf("exposure facade: ok\n");
  return 0;
}
