// policy_set_check.cpp — the argument checks of p2pmg_set_policy_set (csrc/p2pmg_host.cpp::validate_policy_set)
// as a program of its own: no HIP call, no context.  tests/test_cpu_policy_set.py builds it with
// -fsanitize=address,undefined and runs it; it prints "ok <checks>" and exits 0, or names the failed check.
// Every buffer is heap-allocated at its exact size, so a read past a policy or a map is an error, not luck.
#include <cstdio>
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

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

int main() {
  using p2pmg::validate_policy_set;
  const int S = 5, N = 2, A = S * N, NA = 3;
  const size_t NS = 37;  // odd on purpose
  std::string why = "stale";
  std::vector<int32_t> out((size_t)A, -7);

  // the default maps: a (M == A), a % N (M == N), 0 (M == 1), else refused
  {
    std::vector<uint8_t> pol((size_t)A * NS, 0);
    CHECK(validate_policy_set(A, pol.data(), nullptr, NS, NA, N, S, out.data(), &why) == P2PMG_OK && why.empty());
    for (int a = 0; a < A; ++a) CHECK(out[(size_t)a] == a);
    CHECK(validate_policy_set(N, pol.data(), nullptr, NS, NA, N, S, out.data(), &why) == P2PMG_OK);
    for (int a = 0; a < A; ++a) CHECK(out[(size_t)a] == a % N);
    CHECK(validate_policy_set(1, pol.data(), nullptr, NS, NA, N, S, out.data(), &why) == P2PMG_OK);
    for (int a = 0; a < A; ++a) CHECK(out[(size_t)a] == 0);
    for (int m : {3, 4, 7, 9}) {
      CHECK(validate_policy_set(m, pol.data(), nullptr, NS, NA, N, S, out.data(), &why) == P2PMG_E_INVALID);
      CHECK(has(why, "set_policy_set") && has(why, "without policy_of"));
      CHECK(validate_policy_set(m, pol.data(), nullptr, NS, NA, N, S, nullptr, nullptr) == P2PMG_E_INVALID);
    }
    // S = 1: M == A == N, the identity either way; N = 1, M = 1
    CHECK(validate_policy_set(N, pol.data(), nullptr, NS, NA, N, 1, out.data(), &why) == P2PMG_OK);
    CHECK(out[0] == 0 && out[1] == 1);
    CHECK(validate_policy_set(1, pol.data(), nullptr, NS, NA, 1, 1, out.data(), &why) == P2PMG_OK && out[0] == 0);
  }
  // counts
  CHECK(validate_policy_set(0, nullptr, nullptr, NS, NA, N, S, out.data(), &why) == P2PMG_E_INVALID && has(why, "count"));
  CHECK(validate_policy_set(-3, nullptr, nullptr, NS, NA, N, S, nullptr, &why) == P2PMG_E_INVALID);
  // null policies: M empty slots, any M with a map
  {
    std::vector<int32_t> map((size_t)A);
    for (int a = 0; a < A; ++a) map[(size_t)a] = (a * 2) % 3;
    CHECK(validate_policy_set(3, nullptr, map.data(), NS, NA, N, S, out.data(), &why) == P2PMG_OK && why.empty());
    for (int a = 0; a < A; ++a) CHECK(out[(size_t)a] == map[(size_t)a]);
    CHECK(validate_policy_set(3, nullptr, map.data(), NS, NA, N, S, nullptr, nullptr) == P2PMG_OK);
    // entries outside [0, M): the first and the last agent, M itself and a negative one
    for (int at : {0, A - 1}) {
      for (int v : {3, -1, 1 << 30}) {
        std::vector<int32_t> bad = map;
        bad[(size_t)at] = v;
        CHECK(validate_policy_set(3, nullptr, bad.data(), NS, NA, N, S, out.data(), &why) == P2PMG_E_INVALID);
        CHECK(has(why, "policy_of[") && has(why, "outside [0, 3)"));
      }
    }
  }
  // bytes: 0 .. n_actions-1 and 255 are legal, everything else is not, wherever it stands
  {
    const int M = 3;
    std::vector<uint8_t> pol((size_t)M * NS);
    std::vector<int32_t> map((size_t)A, 2);
    const uint8_t legal[4] = {0, 1, 2, P2PMG_POLICY_UNVISITED};
    for (size_t k = 0; k < pol.size(); ++k) pol[k] = legal[k % 4];
    CHECK(validate_policy_set(M, pol.data(), map.data(), NS, NA, N, S, out.data(), &why) == P2PMG_OK);
    for (size_t at : {(size_t)0, NS - 1, NS, pol.size() - 1}) {
      for (int v : {3, 4, 127, 128, 254}) {
        std::vector<uint8_t> bad = pol;
        bad[at] = (uint8_t)v;
        CHECK(validate_policy_set(M, bad.data(), map.data(), NS, NA, N, S, out.data(), &why) == P2PMG_E_INVALID);
        CHECK(has(why, "byte " ) && has(why, std::to_string(v).c_str()) && has(why, ("state " + std::to_string(at % NS)).c_str()));
      }
    }
    // a context of two actions: byte 2 is then illegal, 255 still legal
    CHECK(validate_policy_set(M, pol.data(), map.data(), NS, 2, N, S, out.data(), &why) == P2PMG_E_INVALID);
    std::vector<uint8_t> two(pol.size());
    for (size_t k = 0; k < two.size(); ++k) two[k] = (k % 3 == 2) ? (uint8_t)P2PMG_POLICY_UNVISITED : (uint8_t)(k % 3);
    CHECK(validate_policy_set(M, two.data(), map.data(), NS, 2, N, S, out.data(), &why) == P2PMG_OK);
  }
  // n_states = 0: nothing to read
  {
    std::vector<uint8_t> none;
    CHECK(validate_policy_set(1, none.data(), nullptr, 0, NA, N, S, out.data(), &why) == P2PMG_OK);
  }
  std::printf("ok %d\n", n_checks);
  return 0;
}
