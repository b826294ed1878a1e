"""The native environment switches: the shared helpers of csrc/lpm_env.h against the expressions the launchers held before (a stand-alone host
program under the sanitizers), and docs/switches.md against the code (every LPM_* variable that is read is listed, every listed one is read)."""
import glob
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "learnablepoolingmethods_amd")


def test_env_helper_program_under_the_sanitizers(tmp_path):
    """tools/check_lpm_env.cc: env_int / env_first_is against `e ? atoi(e) : dflt`, `(e && e[0] == ch) ? a : b` and the composed forms for an
    unset variable, "", "0", "1", "2", "junk", "-3", "99999999999", ... -- built with AddressSanitizer and UBSan, a stand-alone host program,
    nothing loaded into Python."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "check_lpm_env")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "check_lpm_env.cc"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '"bad": 0' in r.stdout, r.stdout


def _native_reads():
    names = set()
    for p in glob.glob(os.path.join(PKG, "csrc", "*")):
        names |= set(re.findall(r"\benv_(?:int|first_is|measure_mode)\(\s*\"(LPM_[A-Z0-9_]+)\"", open(p).read()))
    return names


def _python_reads():
    names = set()
    for p in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        names |= set(re.findall(r"os\.environ\.get\(\s*\"(LPM_[A-Z0-9_]+)\"", open(p).read()))
    return names


def test_switch_table_lists_exactly_the_variables_that_are_read():
    for p in glob.glob(os.path.join(PKG, "csrc", "*")):
        if os.path.basename(p) != "lpm_env.h":
            assert "getenv" not in open(p).read(), f"{os.path.basename(p)} reads the environment itself: use csrc/lpm_env.h"
    read = _native_reads() | _python_reads()
    assert len(_native_reads()) == 24 and len(_python_reads()) == 32
    doc = open(os.path.join(ROOT, "docs", "switches.md")).read()
    rows = re.findall(r"^\| `(LPM_[A-Z0-9_]+)` \|.*\| (yes|no) \|$", doc, flags=re.M)
    listed = [n for n, _ in rows]
    assert len(listed) == len(set(listed)), "a variable has two rows"
    assert not sorted(read - set(listed)), f"read in the code, missing from docs/switches.md: {sorted(read - set(listed))}"
    assert not sorted(set(listed) - read), f"listed in docs/switches.md, read nowhere: {sorted(set(listed) - read)}"
    # the measurement column against the code: exactly the variables read between #ifdef LPM_MEASURE and its #else / #endif
    gated = set()
    for p in glob.glob(os.path.join(PKG, "csrc", "*.hip")):
        for block in re.findall(r"^#ifdef LPM_MEASURE\b(.*?)^#(?:else|endif)", open(p).read(), flags=re.S | re.M):
            gated |= set(re.findall(r"\"(LPM_[A-Z0-9_]+)\"", block))
    assert {n for n, m in rows if m == "yes"} == gated
    from learnablepoolingmethods_amd import _capi
    assert set(_capi.MEASURE_VARIABLES) == gated
