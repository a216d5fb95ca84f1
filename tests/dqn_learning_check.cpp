// dqn_learning_check.cpp — the range check of p2pmg_dqn_set_learning (csrc/p2pmg_host.cpp::validate_dqn_learning)
// as a program of its own: no HIP call, no context.  tests/test_cpu_dqn_learning.py builds it with
// -fsanitize=address,undefined and runs it; it prints "ok <checks>" and exits 0, or names the failed check.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "p2pmg.h"
#include "p2pmg_host.h"

static int n_checks = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++n_checks;                                                  \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                  \
    }                                                            \
  } while (0)

int main() {
  using p2pmg::DqnLearn;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const DqnLearn ok{0.95, 0.005, 1e-5, 1.0};
  std::string why = "stale";
  {  // the defaults, the closed ends of the ranges, no rows at all
    std::vector<DqnLearn> rows(3, ok);
    std::vector<float> w(6, 10.0f);
    CHECK(p2pmg::validate_dqn_learning(rows.data(), 3, w.data(), 6, &why) == P2PMG_OK && why.empty());
    rows[1] = DqnLearn{0.0, 0.0, 0.0, 1e-300};
    rows[2] = DqnLearn{1.0, 1.0, 1e9, 1e300};
    w[5] = 0.0f;
    CHECK(p2pmg::validate_dqn_learning(rows.data(), 3, w.data(), 6, &why) == P2PMG_OK && why.empty());
    CHECK(p2pmg::validate_dqn_learning(rows.data(), 3, w.data(), 6, nullptr) == P2PMG_OK);
    CHECK(p2pmg::validate_dqn_learning(nullptr, 0, nullptr, 0, &why) == P2PMG_OK);
  }
  struct Bad {
    DqnLearn row;
    const char* word;
  };
  const Bad bad[] = {{{1.5, 0.005, 1e-5, 1.0}, "gamma"},   {{-0.1, 0.005, 1e-5, 1.0}, "gamma"}, {{nan, 0.005, 1e-5, 1.0}, "gamma"},
                     {{0.95, -0.1, 1e-5, 1.0}, "tau"},     {{0.95, 1.01, 1e-5, 1.0}, "tau"},    {{0.95, inf, 1e-5, 1.0}, "tau"},
                     {{0.95, 0.005, nan, 1.0}, "lr"},      {{0.95, 0.005, -1e-9, 1.0}, "lr"},   {{0.95, 0.005, inf, 1.0}, "lr"},
                     {{0.95, 0.005, 1e-5, 0.0}, "clip"},   {{0.95, 0.005, 1e-5, -1.0}, "clip"}, {{0.95, 0.005, 1e-5, nan}, "clip"},
                     {{0.95, 0.005, 1e-5, inf}, "clip"}};
  for (const Bad& b : bad) {  // the offending network is named, whichever row it is
    for (int at = 0; at < 3; ++at) {
      std::vector<DqnLearn> rows(3, ok);
      std::vector<float> w(3, 10.0f);
      rows[at] = b.row;
      CHECK(p2pmg::validate_dqn_learning(rows.data(), 3, w.data(), 3, &why) == P2PMG_E_INVALID);
      CHECK(why.find(b.word) != std::string::npos && why.find("network " + std::to_string(at)) != std::string::npos);
    }
  }
  for (float v : {-1.0f, -0.0001f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
    std::vector<DqnLearn> rows(1, ok);
    std::vector<float> w(4, 10.0f);
    w[2] = v;
    CHECK(p2pmg::validate_dqn_learning(rows.data(), 1, w.data(), 4, &why) == P2PMG_E_INVALID);
    CHECK(why.find("penalty weight") != std::string::npos && why.find("agent 2") != std::string::npos);
  }
  {  // the first offender wins: a bad row before a bad weight
    std::vector<DqnLearn> rows(2, ok);
    std::vector<float> w(2, -1.0f);
    rows[1].tau = 2.0;
    CHECK(p2pmg::validate_dqn_learning(rows.data(), 2, w.data(), 2, &why) == P2PMG_E_INVALID);
    CHECK(why.find("tau") != std::string::npos && why.find("network 1") != std::string::npos);
  }
  std::printf("ok %d\n", n_checks);
  return 0;
}
