// verdict.hpp — what a host-only rule returns (launch_select.hpp, knobs.hpp). Standard library only.
#pragma once

#include <string>

namespace bsmr {

// a rule's verdict: code 0, or a bsmr_status and the bsmr_last_error text (the caller calls
// set_error: plan.hpp report)
struct Verdict {
    int code = 0;
    std::string msg;
};

}  // namespace bsmr
