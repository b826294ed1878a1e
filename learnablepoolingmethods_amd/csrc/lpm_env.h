// Environment switches of liblpm_hip.so: every native LPM_* variable is read through these (docs/switches.md lists them all).  Plain C++,
// no HIP headers: tools/check_lpm_env.cc builds it alone with a host compiler.  A site keeps the value in a function-local
// `static const`, so the environment is read once per process and never on the launch path.
#pragma once
#include <cstdlib>
#ifdef LPM_MEASURE
#include <cstdio>
#endif

namespace lpm {

// atoi of the variable's value (0 for "" and for text that is no number), or dflt when it is not set
inline int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

// true when the variable is set and its first character is ch
inline bool env_first_is(const char* name, char ch) {
    const char* e = std::getenv(name);
    return e && e[0] == ch;
}

#ifdef LPM_MEASURE
// Measurement builds (-DLPM_MEASURE) only: the value of a variable whose nonzero values select instantiations that skip work, so that
// what the kernel writes is garbage.  Says so once (the caller's `static const`) on stderr.
inline int env_measure_mode(const char* name) {
    const int v = env_int(name, 0);
    if (v) std::fprintf(stderr, "liblpm_hip: %s=%d selects a measurement mode: the results of this process are NOT valid\n", name, v);
    return v;
}
#endif

}  // namespace lpm
