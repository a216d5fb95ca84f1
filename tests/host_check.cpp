// host_check.cpp — stand-alone check of the runtime's HIP-free unit (csrc/p2pmg_host.cpp): the config
// check p2pmg_create makes before its first device call, the default config's constants and the replay
// decoder.  No HIP device is taken.  Every word array handed to the decoder is a heap block of exactly
// the size the call states, so that under -fsanitize=address,undefined a read past it is a report.
// Built and run by tests/test_cpu_host_unit.py; exits 0 and prints "ok <n>" when every case holds.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "p2pmg.h"
#include "p2pmg_host.h"

static int failures = 0, checks = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++checks;                                                        \
    if (!(cond)) {                                                   \
      ++failures;                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
    }                                                                \
  } while (0)

static p2pmg_config defaults() {
  p2pmg_config c;
  CHECK(p2pmg_config_default(&c) == P2PMG_OK);
  return c;
}

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

// The decoder over exact-size heap copies of words and eps, into an exact-size code block filled with
// 0xEE; the status, and codes / consumed as the call left them (consumed starts at 77).
struct Decoded {
  int status;
  std::vector<uint8_t> codes;
  size_t consumed;
};
static Decoded decode(const std::vector<uint32_t>& words, size_t n_decisions, const std::vector<double>& eps) {
  std::unique_ptr<uint32_t[]> w(new uint32_t[words.size()]);
  std::unique_ptr<double[]> e(new double[eps.size()]);
  std::unique_ptr<uint8_t[]> c(new uint8_t[n_decisions]);
  if (!words.empty()) std::memcpy(w.get(), words.data(), words.size() * 4);
  if (!eps.empty()) std::memcpy(e.get(), eps.data(), eps.size() * 8);
  if (n_decisions) std::memset(c.get(), 0xEE, n_decisions);
  Decoded d{0, {}, 77};
  d.status = p2pmg_replay_decode(w.get(), words.size(), n_decisions, e.get(), eps.size(), c.get(), &d.consumed);
  d.codes.assign(c.get(), c.get() + n_decisions);
  return d;
}

// two words whose double is 0 (below any positive epsilon) / the largest below 1 (at or above any epsilon < 1)
static const uint32_t LO0 = 0x0000001Fu, LO1 = 0x0000003Fu;  // the bits the double drops (w0 & 31, w1 & 63) set
static const uint32_t HI = 0xFFFFFFFFu;

int main() {
  CHECK(p2pmg_abi_version() == P2PMG_ABI_VERSION);
  {  // validate_config: what p2pmg_create answers before any device call
    std::string why = "stale";
    p2pmg_config c = defaults();
    CHECK(p2pmg::validate_config(&c, &why) == P2PMG_OK && why.empty());
    CHECK(p2pmg::validate_config(&c, nullptr) == P2PMG_OK);
    CHECK(p2pmg::validate_config(nullptr, &why) == P2PMG_E_INVALID);
    // the table of tests/test_cpu_host.py::test_create_rejects_out_of_range_configs
    struct Row {
      int32_t p2pmg_config::*field;
      int value, status;
    };
    const Row rows[] = {{&p2pmg_config::n_agents, 65, P2PMG_E_UNSUPPORTED}, {&p2pmg_config::n_agents, 0, P2PMG_E_INVALID},
                        {&p2pmg_config::n_scenarios, 0, P2PMG_E_INVALID},  {&p2pmg_config::horizon, 0, P2PMG_E_INVALID},
                        {&p2pmg_config::rounds, -1, P2PMG_E_INVALID},      {&p2pmg_config::rounds, 4096, P2PMG_E_UNSUPPORTED},
                        {&p2pmg_config::n_actions, 4, P2PMG_E_UNSUPPORTED}, {&p2pmg_config::q_dtype, 7, P2PMG_E_INVALID}};
    for (const Row& r : rows) {
      c = defaults();
      c.*r.field = r.value;
      CHECK(p2pmg::validate_config(&c, &why) == r.status && why.empty());
    }
    // the bounds themselves pass
    c = defaults();
    c.n_agents = 64;
    c.rounds = 4095;
    CHECK(p2pmg::validate_config(&c, &why) == P2PMG_OK);
    // 2 actions: a tabular context that only holds tables; no DQN
    c = defaults();
    c.n_actions = 2;
    CHECK(p2pmg::validate_config(&c, &why) == P2PMG_OK && why.empty());
    c.learner = P2PMG_LEARNER_DQN;
    CHECK(p2pmg::validate_config(&c, &why) == P2PMG_E_UNSUPPORTED && why.empty());
    // a Q-network per role is not built: the one refusal with a message
    c = defaults();
    c.shared_q = P2PMG_SHARED_ROLE;
    CHECK(p2pmg::validate_config(&c, &why) == P2PMG_OK && why.empty());
    c.learner = P2PMG_LEARNER_DQN;
    CHECK(p2pmg::validate_config(&c, &why) == P2PMG_E_UNSUPPORTED);
    CHECK(why == "create: shared_q = P2PMG_SHARED_ROLE needs learner = TABULAR (a Q-network per role is not built)");
    CHECK(p2pmg::validate_config(&c, nullptr) == P2PMG_E_UNSUPPORTED);
    c = defaults();
    CHECK(p2pmg::validate_config(&c, &why) == P2PMG_OK && why.empty());  // cleared by the next call
    // an earlier check wins over the message
    c.shared_q = P2PMG_SHARED_ROLE;
    c.learner = P2PMG_LEARNER_DQN;
    c.q_dtype = 7;
    CHECK(p2pmg::validate_config(&c, &why) == P2PMG_E_INVALID && why.empty());
  }
  {  // p2pmg_config_default: the bit patterns tests/test_cpu_host.py pins
    const p2pmg_config c = defaults();
    CHECK(bits(c.inv_ri) == 0x4490ad09u);
    CHECK(bits(c.inv_rvent) == 0x42faa067u);
    CHECK(bits(c.inv_re) == 0x42be79e8u);
    CHECK(bits(c.inv_ci) == 0x345c0771u);
    CHECK(bits(c.inv_cm) == 0x3236c3bbu);
    CHECK(c.n_agents == 2 && c.rounds == 1 && c.horizon == 96 && c.n_actions == 3 && c.learner == P2PMG_LEARNER_TABULAR);
    CHECK(p2pmg_config_default(nullptr) == P2PMG_E_INVALID);
    p2pmg_dqn_config d;
    CHECK(p2pmg_dqn_config_default(&d) == P2PMG_OK && d.batch == 32 && d.capacity == 5000 && d.gamma == 0.95);
    CHECK(p2pmg_dqn_config_default(nullptr) == P2PMG_E_INVALID);
  }
  {  // p2pmg_replay_decode
    // u < eps; the first choice word is 3 (rejected), the second in range: four words read
    Decoded d = decode({LO0, LO1, 0xFFFFFFF7u, 0xABCDEF01u}, 1, {0.5});
    CHECK(d.status == P2PMG_OK && d.codes[0] == 1 && d.consumed == 4);
    d = decode({0, 0, 3, 3, 7, 2, 0x55555555u}, 1, {1e-300});  // three rejections; the word after is not read
    CHECK(d.status == P2PMG_OK && d.codes[0] == 2 && d.consumed == 6);
    // u >= eps: greedy, two words read
    d = decode({HI, HI}, 1, {0.5});
    CHECK(d.status == P2PMG_OK && d.codes[0] == P2PMG_GREEDY && d.consumed == 2);
    d = decode({0x80000000u, 0}, 1, {0.5});  // u == eps exactly is not below it
    CHECK(d.status == P2PMG_OK && d.codes[0] == P2PMG_GREEDY && d.consumed == 2);
    d = decode({0x7FFFFFE0u, 0xFFFFFFC0u, 0}, 1, {0.5});  // the double just below
    CHECK(d.status == P2PMG_OK && d.codes[0] == 0 && d.consumed == 3);
    d = decode({0, 0}, 1, {0.0});  // nothing is below 0
    CHECK(d.status == P2PMG_OK && d.codes[0] == P2PMG_GREEDY && d.consumed == 2);
    // n_eps = 2, cycling: decisions 0 and 2 at eps[0] = 1 explore, decision 1 at eps[1] = 0 does not
    d = decode({0x80000000u, 0, 2, /**/ 0, 0, /**/ 0x12345678u, 0x9ABCDEF0u, 0}, 3, {1.0, 0.0});
    CHECK(d.status == P2PMG_OK && d.consumed == 8);
    CHECK(d.codes[0] == 2 && d.codes[1] == P2PMG_GREEDY && d.codes[2] == 0);
    d = decode({HI, HI, HI, HI, 1, HI, HI, HI, HI, 0}, 4, {0.0, 1.0});  // and the other way round
    CHECK(d.status == P2PMG_OK && d.consumed == 10);
    CHECK(d.codes[0] == P2PMG_GREEDY && d.codes[1] == 1 && d.codes[2] == P2PMG_GREEDY && d.codes[3] == 0);
    // the input ends after one word of a double
    d = decode({0}, 1, {0.5});
    CHECK(d.status == P2PMG_E_INVALID && d.consumed == 77);
    d = decode({HI, HI, 0}, 2, {0.5});  // ... of the second decision's: the first is decoded
    CHECK(d.status == P2PMG_E_INVALID && d.codes[0] == P2PMG_GREEDY && d.codes[1] == 0xEE);
    d = decode({}, 1, {0.5});
    CHECK(d.status == P2PMG_E_INVALID);
    // the input ends inside the rejection loop
    d = decode({0, 0}, 1, {0.5});
    CHECK(d.status == P2PMG_E_INVALID && d.codes[0] == 0xEE);
    d = decode({0, 0, 3}, 1, {0.5});
    CHECK(d.status == P2PMG_E_INVALID && d.codes[0] == 0xEE);
    d = decode({0, 0, 3, 7, 0xFFFFFFFFu}, 1, {0.5});
    CHECK(d.status == P2PMG_E_INVALID && d.consumed == 77);
    // no decisions: nothing is read or written
    d = decode({}, 0, {0.5});
    CHECK(d.status == P2PMG_OK && d.consumed == 0);
    d = decode({1, 2, 3}, 0, {0.5});
    CHECK(d.status == P2PMG_OK && d.consumed == 0);
    // consumed is optional; null arrays and an empty epsilon list are refused
    const uint32_t w[2] = {HI, HI};
    const double e = 0.5;
    uint8_t code = 0xEE;
    CHECK(p2pmg_replay_decode(w, 2, 1, &e, 1, &code, nullptr) == P2PMG_OK && code == P2PMG_GREEDY);
    CHECK(p2pmg_replay_decode(nullptr, 2, 1, &e, 1, &code, nullptr) == P2PMG_E_INVALID);
    CHECK(p2pmg_replay_decode(w, 2, 1, nullptr, 1, &code, nullptr) == P2PMG_E_INVALID);
    CHECK(p2pmg_replay_decode(w, 2, 1, &e, 0, &code, nullptr) == P2PMG_E_INVALID);
    CHECK(p2pmg_replay_decode(w, 2, 1, &e, 1, nullptr, nullptr) == P2PMG_E_INVALID);
  }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
