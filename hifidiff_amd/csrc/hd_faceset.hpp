// hd_faceset.hpp -- FaceSet: the host's copy of one per-face flag of the prepared batch ("carries a mask", "is guided", "has a multistep
// history"): the batch it was sized for, the flags, and how many are set.  Nothing here needs HIP: tests/test_face_state_host.py compiles
// this header alone with the host compiler.
#pragma once
#include <cstddef>
#include <vector>

namespace hdi {

class FaceSet {
public:
    void reset(int B) { flags_.assign((size_t)B, 0); B_ = B; count_ = 0; }    // all clear, sized for B
    void drop() { reset(0); }                                                 // sized for no batch
    bool valid_for(int B) const { return B > 0 && B == B_; }
    void set(int slot, bool on) { count_ += (on ? 1 : 0) - flags_[(size_t)slot]; flags_[(size_t)slot] = on ? 1 : 0; }
    bool get(int slot) const { return flags_[(size_t)slot] != 0; }
    int count() const { return count_; }
    bool any(int B) const { return valid_for(B) && count_ > 0; }
    bool all(int B) const { return valid_for(B) && count_ == B; }

private:
    std::vector<char> flags_;
    int B_ = 0, count_ = 0;
};

}  // namespace hdi
