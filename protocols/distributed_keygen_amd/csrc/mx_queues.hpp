// Hardware-queue policy of mx_configure_hw_queues (include/mxpaillier.h): what a request, the inherited value of
// GPU_MAX_HW_QUEUES and the opt-out add up to.  Host code only, no HIP and no environment access: the caller reads
// and writes the environment, so that the decision itself is testable without a device (tools/hw_queue_policy_check.cpp).
#pragma once
#include <cerrno>
#include <cstdlib>

namespace mxq {

constexpr int MIN_HW_QUEUES = 1;
constexpr int MAX_HW_QUEUES = 32;      // the library never WRITES more than this, whatever is requested

inline int clamp_request(int queues) {
  return queues < MIN_HW_QUEUES ? MIN_HW_QUEUES : queues > MAX_HW_QUEUES ? MAX_HW_QUEUES : queues;
}

// A value of the variable as a positive decimal number (blanks around it allowed); 0 for unset, empty or anything
// else — "4x", "-2", "0", a number beyond int —, which counts as unset.
inline int parse_queues(const char* text) {
  if (!text) return 0;
  while (*text == ' ' || *text == '\t') ++text;
  if (*text < '0' || *text > '9') return 0;
  errno = 0;
  char* end = nullptr;
  const long v = std::strtol(text, &end, 10);
  while (*end == ' ' || *end == '\t') ++end;
  if (*end != '\0' || errno != 0 || v <= 0 || v > 1000000) return 0;
  return (int)v;
}

struct QueueDecision {
  int value;      // what the environment holds once the decision is carried out (0: unset, the runtime's own default)
  bool write;     // true: the caller sets the variable to `value`
};

// `inherited` is the variable's text (NULL = unset), `keep` the opt-out (MX_HW_QUEUES_KEEP=1: change nothing).
// A request is clamped to 1..32 and written only when the variable is unset, unreadable or smaller: a larger
// inherited value stays, also one above 32 — the library does not set it, the user did.
inline QueueDecision decide_hw_queues(int request, const char* inherited, bool keep) {
  const int have = parse_queues(inherited);
  if (keep) return QueueDecision{have, false};
  const int want = clamp_request(request);
  if (have >= want) return QueueDecision{have, false};
  return QueueDecision{want, true};
}

// MX_HW_QUEUES_KEEP counts as set only when it is exactly "1".
inline bool keep_requested(const char* text) { return text && text[0] == '1' && text[1] == '\0'; }

}  // namespace mxq
