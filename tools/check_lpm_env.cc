// Host check of the environment-switch helpers (learnablepoolingmethods_amd/csrc/lpm_env.h) against the expressions the launchers held before
// they shared them: `e ? atoi(e) : dflt`, `(e && e[0] == ch) ? a : b`, and the composed forms (a range with a fall-back, a two-bit mask).
//     c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_lpm_env.cc -o check_lpm_env
//     ./check_lpm_env
// Every case sets the variable with setenv (or removes it) and compares.  Prints one JSON line; exit status 0 when nothing differs.
#include "../learnablepoolingmethods_amd/csrc/lpm_env.h"

#include <cstdio>

namespace {

const char* kName = "LPM_CHECK_ENV_VARIABLE";

// the old forms, as they stood at the sites
int old_int(int dflt) { const char* e = std::getenv(kName); return e ? std::atoi(e) : dflt; }
int old_first(char ch, int yes, int no) { const char* e = std::getenv(kName); return (e && e[0] == ch) ? yes : no; }
int old_range(int lo, int hi, int dflt) { const char* e = std::getenv(kName); const int v = e ? std::atoi(e) : 0; return (v >= lo && v <= hi) ? v : dflt; }
int old_kb() { const char* e = std::getenv(kName); const int v = e ? std::atoi(e) : 0; return (v == 1 || v == 2 || v == 4) ? v : 2; }
int old_mask(int dflt) { const char* e = std::getenv(kName); return e ? (std::atoi(e) & 3) : dflt; }

int new_range(int lo, int hi, int dflt) { const int v = lpm::env_int(kName, 0); return (v >= lo && v <= hi) ? v : dflt; }
int new_kb() { const int v = lpm::env_int(kName, 0); return (v == 1 || v == 2 || v == 4) ? v : 2; }

int check(const char* value) {
    if (value) setenv(kName, value, 1);
    else unsetenv(kName);
    int bad = 0;
    const int dflts[] = {0, 1, 8, 32, -7};
    const char firsts[] = {'0', '1', '2', '3', 'j', '-'};
    for (int dflt : dflts) bad += lpm::env_int(kName, dflt) != old_int(dflt);
    for (char ch : firsts) {
        bad += (lpm::env_first_is(kName, ch) ? 0 : 1) != old_first(ch, 0, 1);      // "0" switches off
        bad += (lpm::env_first_is(kName, ch) ? 1 : 0) != old_first(ch, 1, 0);      // "1" switches on
        bad += (lpm::env_first_is(kName, ch) ? 3 : 4) != old_first(ch, 3, 4);      // one of two integers
    }
    bad += new_range(4, 5, 4) != old_range(4, 5, 4);
    bad += new_kb() != old_kb();
    bad += (lpm::env_int(kName, 0) & 3) != old_mask(0);
    if (bad) std::fprintf(stderr, "mismatch for %s%s%s\n", value ? "\"" : "", value ? value : "unset", value ? "\"" : "");
    return bad;
}

}  // namespace

int main() {
    const char* values[] = {nullptr, "", "0", "1", "2", "junk", "-3", "99999999999", "3", "4", "5", "8", "07", " 1"};
    int bad = 0, cases = 0;
    for (const char* v : values) {
        bad += check(v);
        ++cases;
    }
    // the fixed points the sites rely on
    unsetenv(kName);
    bad += lpm::env_int(kName, 32) != 32 || lpm::env_first_is(kName, '0');
    setenv(kName, "", 1);
    bad += lpm::env_int(kName, 32) != 0 || lpm::env_first_is(kName, '0');
    setenv(kName, "junk", 1);
    bad += lpm::env_int(kName, 8) != 0 || !lpm::env_first_is(kName, 'j');
    setenv(kName, "-3", 1);
    bad += lpm::env_int(kName, 0) != -3 || (lpm::env_int(kName, 0) & 3) != 1;
    std::printf("{\"cases\": %d, \"bad\": %d}\n", cases, bad);
    return bad ? 1 : 0;
}
