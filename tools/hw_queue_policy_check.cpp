// Stand-alone check of the hardware-queue policy of mx_configure_hw_queues (protocols/distributed_keygen_amd/csrc/
// mx_queues.hpp): the decision function over the cases of tests/test_hw_queue_policy.py, carried out on this process's
// own environment the way the library does it.  Host code only, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/hw_queue_policy_check.cpp -o /tmp/hw_queue_policy_check
//   /tmp/hw_queue_policy_check          (prints "hw queue policy ok", exit status 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../protocols/distributed_keygen_amd/csrc/mx_queues.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

// the library's steps around the decision: read, decide, write, report
int configure(int request) {
  const mxq::QueueDecision d = mxq::decide_hw_queues(request, std::getenv("GPU_MAX_HW_QUEUES"),
                                                     mxq::keep_requested(std::getenv("MX_HW_QUEUES_KEEP")));
  if (d.write) setenv("GPU_MAX_HW_QUEUES", std::to_string(d.value).c_str(), 1);
  return d.value;
}

void start(const char* inherited, const char* keep) {
  if (inherited) setenv("GPU_MAX_HW_QUEUES", inherited, 1); else unsetenv("GPU_MAX_HW_QUEUES");
  if (keep) setenv("MX_HW_QUEUES_KEEP", keep, 1); else unsetenv("MX_HW_QUEUES_KEEP");
}

bool env_is(const char* want) {
  const char* have = std::getenv("GPU_MAX_HW_QUEUES");
  return want ? (have && std::strcmp(have, want) == 0) : have == nullptr;
}

}  // namespace

int main() {
  // parsing: a positive decimal number or nothing
  expect(mxq::parse_queues(nullptr) == 0 && mxq::parse_queues("") == 0 && mxq::parse_queues("  ") == 0, "unset / empty / blank parse as 0");
  expect(mxq::parse_queues("4") == 4 && mxq::parse_queues(" 24\t") == 24 && mxq::parse_queues("007") == 7, "numbers parse");
  expect(mxq::parse_queues("4x") == 0 && mxq::parse_queues("x4") == 0 && mxq::parse_queues("-2") == 0 && mxq::parse_queues("+4") == 0 &&
         mxq::parse_queues("0") == 0 && mxq::parse_queues("4 4") == 0 && mxq::parse_queues("1e3") == 0, "garbage parses as 0");
  expect(mxq::parse_queues("99999999999999999999999999") == 0 && mxq::parse_queues("1000001") == 0, "numbers out of range parse as 0");
  expect(mxq::clamp_request(0) == 1 && mxq::clamp_request(-7) == 1 && mxq::clamp_request(1) == 1 && mxq::clamp_request(32) == 32 &&
         mxq::clamp_request(33) == 32 && mxq::clamp_request(2147483647) == 32 && mxq::clamp_request(-2147483647 - 1) == 1, "clamp to 1..32");
  expect(mxq::keep_requested("1") && !mxq::keep_requested(nullptr) && !mxq::keep_requested("") && !mxq::keep_requested("0") &&
         !mxq::keep_requested("11") && !mxq::keep_requested("yes"), "the opt-out is exactly 1");

  start(nullptr, nullptr);
  expect(configure(16) == 16 && env_is("16"), "unset -> 16");
  start("4", nullptr);
  expect(configure(16) == 16 && env_is("16"), "inherited 4 -> 16");
  start("24", nullptr);
  expect(configure(16) == 24 && env_is("24"), "inherited 24 stays");
  start(nullptr, nullptr);
  expect(configure(64) == 32 && env_is("32"), "request 64 -> 32");
  start("4", nullptr);
  expect(configure(64) == 32 && env_is("32"), "request 64 over inherited 4 -> 32");
  start("48", nullptr);
  expect(configure(64) == 48 && env_is("48"), "an inherited value above 32 is not the library's to change");
  start(nullptr, nullptr);
  expect(configure(0) == 1 && env_is("1"), "request 0 -> 1");
  start(nullptr, nullptr);
  expect(configure(-5) == 1 && env_is("1"), "negative request -> 1");
  start("4", nullptr);
  expect(configure(0) == 4 && env_is("4"), "request 0 under inherited 4 changes nothing");
  start("4", "1");
  expect(configure(16) == 4 && env_is("4"), "MX_HW_QUEUES_KEEP=1 with inherited 4 -> 4");
  start(nullptr, "1");
  expect(configure(16) == 0 && env_is(nullptr), "MX_HW_QUEUES_KEEP=1 with nothing inherited leaves it unset");
  start("4", "0");
  expect(configure(16) == 16 && env_is("16"), "MX_HW_QUEUES_KEEP=0 is no opt-out");
  start("lots", nullptr);
  expect(configure(16) == 16 && env_is("16"), "inherited garbage counts as unset");
  start("", nullptr);
  expect(configure(16) == 16 && env_is("16"), "an empty value counts as unset");
  start("4", nullptr);
  expect(configure(16) == 16 && configure(8) == 16 && env_is("16"), "a second, smaller request does not lower the value");
  start("4", nullptr);
  expect(configure(8) == 8 && configure(16) == 16 && env_is("16"), "a second, larger request raises it");
  for (int request = -40; request <= 80; ++request) {          // whatever is asked for, nothing above 32 is ever written
    start("2", nullptr);
    const int got = configure(request);
    expect(got >= 2 && got <= 32 && mxq::parse_queues(std::getenv("GPU_MAX_HW_QUEUES")) == got, "sweep of requests over inherited 2");
  }
  if (failures) return 1;
  std::puts("hw queue policy ok");
  return 0;
}
