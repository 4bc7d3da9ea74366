"""Lanes (barc4dip_amd/csrc/b4d_lanes.hpp), the fork / join of the two-lane launch groups, as host code: a stand-alone C++
program with its own main, built against a recording stand-in for <hip/hip_runtime.h>.  The stand-in implements the event and
stream calls Lanes makes (and declares the few names b4d_common.hpp mentions); every call is appended to a log and a switch makes
the n-th call fail.  No GPU, nothing loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_STANDIN = r"""
#pragma once
#include <cstddef>
#include <string>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorUnknown = 999;
struct StandinStream { const char* name; };
struct StandinEvent { int id; bool recorded; };
typedef StandinStream* hipStream_t;
typedef StandinEvent* hipEvent_t;
constexpr unsigned hipEventDisableTiming = 2;
struct dim3 { unsigned x, y, z; };
hipError_t hipGetLastError();   // named by launch() (b4d_common.hpp), never called here

extern std::vector<std::string> g_log;   // one entry per call, failed ones included
extern int g_fail_at;                    // the call that makes the log this long fails; 0: none

inline hipError_t standin_call(const std::string& what) {
    g_log.push_back(what);
    return g_fail_at && (int)g_log.size() == g_fail_at ? hipErrorUnknown : hipSuccess;
}
inline const char* hipGetErrorString(hipError_t) { return "stand-in failure"; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    static int made = 0;
    const hipError_t rc = standin_call("create");
    if (rc == hipSuccess) *e = new StandinEvent{++made, false};
    return rc;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    const hipError_t rc = standin_call("record e" + std::to_string(e->id) + " on " + (s ? s->name : "null"));
    if (rc == hipSuccess) e->recorded = true;
    return rc;
}
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    return standin_call(std::string(s ? s->name : "null") + " waits e" + std::to_string(e->id) + (e->recorded ? "" : " UNRECORDED"));
}
"""

LANES_PROGRAM = r"""
#include <cstdio>
#include <type_traits>

#include "b4d_lanes.hpp"

std::vector<std::string> g_log;
int g_fail_at = 0;
static StandinStream s_caller{"caller"}, s_aux{"aux"};
static int g_lane_streams = 0;

namespace b4d {   // what b4d_kernels.hip defines in the library
std::string& last_error() {
    static std::string err;
    return err;
}
std::atomic<int> g_opt_lanes{1};
int lane_stream(int, hipStream_t* out) {
    ++g_lane_streams;
    *out = &s_aux;
    return B4D_OK;
}
}  // namespace b4d

static long bad = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            ++bad;                                                    \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            for (const std::string& l : g_log) std::printf("    %s\n", l.c_str()); \
        }                                                             \
    } while (0)

static void reset() {
    g_log.clear();
    g_fail_at = 0;
    b4d::last_error().clear();
}
static void free_events(LaneSync& ls) {
    delete ls.ev_fork;
    delete ls.ev_join;
}

int main() {
    static_assert(!std::is_copy_constructible<Lanes>::value && !std::is_copy_assignable<Lanes>::value, "Lanes is not copyable");
    const std::vector<std::string> fork_log{"create", "create", "record e1 on caller", "aux waits e1"};
    const std::vector<std::string> full_log{"create", "create", "record e1 on caller", "aux waits e1", "record e2 on aux", "caller waits e2"};
    LaneSync ls;
    {   // 1. fork -> groups -> close(): fork-wait and join-wait once each, in that order
        Lanes ln;
        CHECK(ln.fork(ls, &s_caller, true) == B4D_OK && ln.two);
        CHECK(g_log == fork_log && g_lane_streams == 1);
        CHECK(ln.stream(0) == &s_caller && ln.stream(1) == &s_aux && ln.stream(2) == &s_caller && ln.slot(0) == 0 && ln.slot(3) == 1);
        CHECK(ln.close() == B4D_OK);
        CHECK(g_log == full_log);
        CHECK(ln.close() == B4D_OK && g_log == full_log);   // idempotent
    }
    CHECK(g_log == full_log);   // 4. close() followed by the destructor joins once
    CHECK(ls.aux == &s_aux && ls.ev_fork && ls.ev_fork->id == 1 && ls.ev_join && ls.ev_join->id == 2);

    reset();
    {   // 2. a scope left early after a successful two-lane fork still joins, exactly once; stream and events are reused
        Lanes ln;
        CHECK(ln.fork(ls, &s_caller, true) == B4D_OK);
        b4d::last_error() = "the failure that ends the scope";
    }
    CHECK((g_log == std::vector<std::string>{"record e1 on caller", "aux waits e1", "record e2 on aux", "caller waits e2"}));
    CHECK(g_lane_streams == 1 && b4d::last_error() == "the failure that ends the scope");

    reset();
    {   // the destructor is best effort: a failing record is not waited on, and last_error() keeps the caller's message
        Lanes ln;
        CHECK(ln.fork(ls, &s_caller, true) == B4D_OK);
        b4d::last_error() = "first failure";
        g_fail_at = 3;
    }
    CHECK(g_log.size() == 3 && g_log.back() == "record e2 on aux" && b4d::last_error() == "first failure");

    reset();
    {   // a join that fails inside close() surfaces there and is not tried again
        Lanes ln;
        CHECK(ln.fork(ls, &s_caller, true) == B4D_OK);
        g_fail_at = 3;
        CHECK(ln.close() == B4D_EHIP && !b4d::last_error().empty());
    }
    CHECK(g_log.size() == 3);

    reset();
    {   // 3. a one-lane Lanes records nothing: not asked for, or option "lanes" 0
        Lanes a;
        CHECK(a.fork(ls, &s_caller, false) == B4D_OK && !a.two && a.stream(1) == &s_caller && a.slot(1) == 0);
        CHECK(a.close() == B4D_OK);
        b4d::g_opt_lanes = 0;
        Lanes b;
        CHECK(b.fork(ls, &s_caller, true) == B4D_OK && !b.two);
        Lanes c;   // open(): 8 frames of 1 MiB against groups of at least 8 MiB stay on one lane, in the plan's own groups
        CHECK(c.open(ls, 4, &s_caller, 8, (size_t)1 << 20, (size_t)1 << 20, true, (size_t)8 << 20) == B4D_OK && !c.two && c.sub == 4);
        b4d::g_opt_lanes = 1;
        Lanes d;   // never forked at all
    }
    CHECK(g_log.empty());

    reset();
    {   // open(): 32-MiB intermediates -> 2 frames per group, an even number of equal groups, forked
        Lanes ln, one;
        CHECK(ln.open(ls, 8, &s_caller, 14, (size_t)32 << 20, (size_t)16 << 20, true, (size_t)8 << 20) == B4D_OK && ln.two && ln.sub == 2);
        CHECK(one.open(ls, 8, &s_caller, 1, (size_t)32 << 20, (size_t)16 << 20, true, (size_t)8 << 20) == B4D_OK && !one.two && one.sub == 8);
    }
    CHECK(g_log.size() == 4);   // one fork, one join

    // 5. a failing event call inside fork surfaces as B4D_EHIP, and the destructor then waits on nothing (least of all on an
    // event that was never recorded): every call of a first fork in turn
    for (int n = 1; n <= 4; ++n) {
        reset();
        LaneSync fresh;
        {
            Lanes ln;
            g_fail_at = n;
            CHECK(ln.fork(fresh, &s_caller, true) == B4D_EHIP);
            CHECK((int)g_log.size() == n && !b4d::last_error().empty());
            g_fail_at = 0;
        }
        CHECK((int)g_log.size() == n);
        for (const std::string& l : g_log) CHECK(l.find("UNRECORDED") == std::string::npos && l.find("caller waits") == std::string::npos);
        free_events(fresh);
    }
    free_events(ls);
    std::printf("TOTAL BAD %ld\n", bad);
    return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def lanes_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("lanes_host")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STANDIN)
    src, exe = d / "lanes.cpp", d / "lanes"
    src.write_text(LANES_PROGRAM)
    # a stand-alone program with its own main: the sanitizers are linked in the ordinary way
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", str(d), "-I", os.path.join(ROOT, "barc4dip_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:      # a compiler without the sanitizer runtimes still checks the protocol
        r = subprocess.run([c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_lanes_join_on_every_exit(lanes_program):
    """fork -> groups -> close() records fork-wait and join-wait once each, in that order; a scope left early after a two-lane
    fork still joins exactly once (and leaves last_error() alone); a one-lane Lanes records nothing; close() followed by the
    destructor joins once; a failing event call inside fork is B4D_EHIP and the destructor then waits on no event."""
    r = subprocess.run([lanes_program], capture_output=True, text=True)
    assert r.returncode == 0 and "TOTAL BAD 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
