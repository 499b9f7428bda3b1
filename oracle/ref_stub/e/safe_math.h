// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_hash.so).
// Stand-in for libe's <e/safe_math.h>: checked int64 arithmetic, true on
// success.  Only datatype_int64::apply calls these; the hash path never does.
#ifndef e_safe_math_h_
#define e_safe_math_h_
#include <stdint.h>

namespace e {

inline bool safe_add(int64_t a, int64_t b, int64_t* r) { return !__builtin_add_overflow(a, b, r); }
inline bool safe_sub(int64_t a, int64_t b, int64_t* r) { return !__builtin_sub_overflow(a, b, r); }
inline bool safe_mul(int64_t a, int64_t b, int64_t* r) { return !__builtin_mul_overflow(a, b, r); }

inline bool safe_div(int64_t a, int64_t b, int64_t* r) {
    if (b == 0 || (a == INT64_MIN && b == -1)) return false;
    *r = a / b;
    return true;
}

inline bool safe_mod(int64_t a, int64_t b, int64_t* r) {
    if (b == 0 || (a == INT64_MIN && b == -1)) return false;
    *r = a % b;
    return true;
}

}  // namespace e
#endif
