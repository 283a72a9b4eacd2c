// store_policy_check.cpp -- the frame stores' cache policy on the CPU: the
// per-device record of recent frame targets (rt_dispatch::track_target) and
// the choice choose() makes from the working set it returns.  A stand-alone
// program like tests/dispatch_check.cpp: tests/test_store_policy.py builds it
// next to rt_dispatch.cpp and rt_args.cpp with -fsanitize=address,undefined
// and runs it (-fsanitize=thread builds it too, for the two-thread case).
// No GPU, no HIP.  Every expected value is a literal worked out by hand.
// Exit 0 and "store policy check ok" on success.
#include <cstdint>
#include <cstdio>
#include <thread>

#include "rt_dispatch.h"
#include "rt_hip.h"
#include "rt_hip_debug.h"

namespace {

using rt_dispatch::Decision;
using rt_dispatch::Geometry;
using rt_dispatch::Knobs;
using rt_dispatch::reset_targets;
using rt_dispatch::track_target;

int failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, \
                         #cond);                                                 \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

constexpr int64_t MiB = (int64_t)1 << 20;
// addresses only: nothing is ever read or written through them
const void* at(int64_t mib) { return reinterpret_cast<const void*>((uintptr_t)(mib * MiB)); }

void same_buffer_counts_once() {
    reset_targets();
    for (int i = 0; i < 20; ++i) CHECK(track_target(0, at(1024), 256 * MiB) == 256 * MiB);
}

void two_buffers_sum() {
    reset_targets();
    CHECK(track_target(0, at(1024), 256 * MiB) == 256 * MiB);
    CHECK(track_target(0, at(2048), 256 * MiB) == 512 * MiB);
    // alternating keeps both, however long
    for (int i = 0; i < 20; ++i) {
        CHECK(track_target(0, at(1024), 256 * MiB) == 512 * MiB);
        CHECK(track_target(0, at(2048), 256 * MiB) == 512 * MiB);
    }
    // a third of another size joins them; an empty one adds nothing
    CHECK(track_target(0, at(4096), 64 * MiB) == 576 * MiB);
    CHECK(track_target(0, at(8192), 0) == 576 * MiB);
}

void entries_age_out() {
    static_assert(rt_dispatch::kTargetWindow == 8, "the counts below are for a window of 8");
    reset_targets();
    CHECK(track_target(0, at(1024), 256 * MiB) == 256 * MiB);  // render 1
    // renders 2..8 of another buffer: render 1 is still among the last 8
    for (int i = 2; i <= 8; ++i) CHECK(track_target(0, at(2048), 100 * MiB) == 356 * MiB);
    // render 9: the last 8 are renders 2..9, all of the second buffer
    CHECK(track_target(0, at(2048), 100 * MiB) == 100 * MiB);
    // eight distinct targets in a row all count; the ninth pushes the first out
    reset_targets();
    for (int i = 1; i <= 8; ++i) CHECK(track_target(0, at(1024 * i), 10 * MiB) == i * 10 * MiB);
    CHECK(track_target(0, at(1024 * 9), 10 * MiB) == 80 * MiB);
    // the same base with another length is another target; the old one ages out
    reset_targets();
    CHECK(track_target(0, at(1024), 64 * MiB) == 64 * MiB);
    CHECK(track_target(0, at(1024), 32 * MiB) == 64 * MiB);  // inside the first: the union
    for (int i = 0; i < 6; ++i) CHECK(track_target(0, at(1024), 32 * MiB) == 64 * MiB);
    CHECK(track_target(0, at(1024), 32 * MiB) == 32 * MiB);
}

void overlaps_count_once() {
    reset_targets();
    CHECK(track_target(0, at(1000), 100 * MiB) == 100 * MiB);  // [1000, 1100)
    CHECK(track_target(0, at(1050), 100 * MiB) == 150 * MiB);  // [1050, 1150)
    CHECK(track_target(0, at(1020), 10 * MiB) == 150 * MiB);   // inside
    CHECK(track_target(0, at(1150), 50 * MiB) == 200 * MiB);   // adjacent: [1150, 1200)
    CHECK(track_target(0, at(900), 400 * MiB) == 400 * MiB);   // covers them all
    CHECK(track_target(0, at(2000), 1 * MiB) == 401 * MiB);    // disjoint
    // the bands of one frame, rendered one by one, are the frame
    reset_targets();
    for (int b = 0; b < 4; ++b) CHECK(track_target(0, at(1024 + 64 * b), 64 * MiB) == 64 * MiB * (b + 1));
}

void devices_are_separate() {
    reset_targets();
    CHECK(track_target(0, at(1024), 256 * MiB) == 256 * MiB);
    CHECK(track_target(1, at(1024), 256 * MiB) == 256 * MiB);
    CHECK(track_target(1, at(2048), 256 * MiB) == 512 * MiB);
    CHECK(track_target(0, at(1024), 256 * MiB) == 256 * MiB);
    CHECK(track_target(7, at(4096), 1 * MiB) == 1 * MiB);
    // a device's renders do not age another's targets
    for (int i = 0; i < 20; ++i) track_target(1, at(2048), 256 * MiB);
    CHECK(track_target(0, at(2048), 256 * MiB) == 512 * MiB);
}

void two_threads() {
    reset_targets();
    // each thread alternates between its own two buffers on the shared device
    // 0 and renders to one of its own on device 1 + t; whatever the
    // interleaving, a call sees its own target and at most the four of device 0
    int bad[2] = {0, 0};
    auto work = [&bad](int t) {
        for (int i = 0; i < 20000; ++i) {
            const int64_t ws = track_target(0, at(1024 * (1 + 2 * t + (i & 1))), 16 * MiB);
            if (ws < 16 * MiB || ws > 64 * MiB || ws % (16 * MiB) != 0) ++bad[t];
            if (track_target(1 + t, at(1024), 8 * MiB) != 8 * MiB) ++bad[t];
        }
    };
    std::thread a(work, 0), b(work, 1);
    a.join();
    b.join();
    CHECK(bad[0] == 0 && bad[1] == 0);
    // afterwards the record is still consistent
    CHECK(track_target(1, at(1024), 8 * MiB) == 8 * MiB);
    const int64_t ws = track_target(0, at(1024), 16 * MiB);
    CHECK(ws >= 16 * MiB && ws <= 64 * MiB);
}

// rt_trace.inc's kGeometry of the 16x16 build (tests/dispatch_check.cpp)
const Geometry G16{64, 64, 16, 2, 64, 4, 2, 8, 1024, 4096, 128, 32, 32, 48};

int policy(const Knobs& k, int32_t fmt, int ns, int nc, int32_t w, int32_t h, unsigned verdict,
           int64_t working_set, int* chain = nullptr) {
    Decision dc;
    const int rc = rt_dispatch::choose(G16, k, 256, fmt, ns, nc, w, h, true, RT_PATH_AUTO, verdict,
                                       0, &dc, working_set);
    CHECK(rc == RT_OK);
    if (chain) *chain = dc.chain;
    return dc.store_policy;
}

void choice() {
    Knobs k;
    CHECK(k.store_policy == RT_STORE_AUTO && k.store_large_bytes == 512 * MiB);
    CHECK(rt_dispatch::kStoreLargeBytes == 512 * MiB);
    int chain = 0;
    // config 3: 4096 x 4096 int32x4 = 256 MiB, trace_bin_kernel (verdict 2)
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 4096, 4096, 2, 0, &chain) == RT_STORE_DEFAULT);
    CHECK(chain == RT_KERNEL_TRACE_BIN);
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 4096, 4096, 2, 256 * MiB) == RT_STORE_DEFAULT);
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 4096, 4096, 2, 512 * MiB - 1) == RT_STORE_DEFAULT);
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 4096, 4096, 2, 512 * MiB) == RT_STORE_LARGE);
    // a nearly empty frame (verdict 1) keeps the default, unless forced
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 4096, 4096, 1, 512 * MiB, &chain) == RT_STORE_DEFAULT);
    CHECK(chain == RT_KERNEL_TRACE_BIN);
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 8192, 8192, 1, 0) == RT_STORE_DEFAULT);
    // ... and on the coarse chain's trace3_kernel (no verdict yet)
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 4096, 4096, 0, 512 * MiB, &chain) == RT_STORE_LARGE);
    CHECK(chain == RT_KERNEL_TRACE);
    // a single target of 512 MiB is the old frame-size rule: 8192 x 4096 x 16 B
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 8192, 4096, 2, 0) == RT_STORE_LARGE);
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 8192, 4095, 2, 0) == RT_STORE_DEFAULT);
    // a working set below the frame's own bytes means the frame alone
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 8192, 4096, 2, 1 * MiB) == RT_STORE_LARGE);
    // RGBA8: four 64 MiB frames in flight stay below, eight reach it
    CHECK(policy(k, RT_FORMAT_RGBA8, 256, 64, 4096, 4096, 2, 256 * MiB) == RT_STORE_DEFAULT);
    CHECK(policy(k, RT_FORMAT_RGBA8, 256, 64, 4096, 4096, 2, 512 * MiB) == RT_STORE_LARGE);
    CHECK(policy(k, RT_FORMAT_HIT, 256, 64, 4096, 4096, 3, 512 * MiB) == RT_STORE_LARGE);
    // the split trace has the policy too: 1024 x 1024, two waves per tile
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 1024, 1024, 0, 512 * MiB, &chain) == RT_STORE_LARGE);
    CHECK(chain == RT_KERNEL_TRACE_SPLIT);
    // the small-scene kernels have one policy, whatever the working set
    CHECK(policy(k, RT_FORMAT_I32X4, 16, 4, 640, 480, 0, 4096 * MiB, &chain) == RT_STORE_DEFAULT);
    CHECK(chain == RT_KERNEL_FRAME_SMALL);
    CHECK(policy(k, RT_FORMAT_I32X4, 16, 4, 4096, 4096, 0, 4096 * MiB, &chain) == RT_STORE_DEFAULT);
    CHECK(chain == RT_KERNEL_TRACE_SMALL);
    // rt_debug_set_store_large_bytes
    k.store_large_bytes = 1000;
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 8, 8, 0, 0) == RT_STORE_LARGE);  // 1024 B
    CHECK(policy(k, RT_FORMAT_RGBA8, 256, 64, 8, 8, 0, 0) == RT_STORE_DEFAULT);  // 256 B
    CHECK(policy(k, RT_FORMAT_RGBA8, 256, 64, 8, 8, 0, 1000) == RT_STORE_LARGE);
    // rt_debug_set_store_policy forces either
    k = Knobs{};
    k.store_policy = RT_STORE_LARGE;
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 64, 64, 0, 0) == RT_STORE_LARGE);
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 4096, 4096, 1, 0) == RT_STORE_LARGE);
    k.store_policy = RT_STORE_DEFAULT;
    CHECK(policy(k, RT_FORMAT_I32X4, 256, 64, 8192, 8192, 2, 4096 * MiB) == RT_STORE_DEFAULT);
    // store_policy_of by itself
    k = Knobs{};
    CHECK(rt_dispatch::store_policy_of(k, 256 * MiB, 0, 2) == RT_STORE_DEFAULT);
    CHECK(rt_dispatch::store_policy_of(k, 256 * MiB, 512 * MiB, 2) == RT_STORE_LARGE);
    CHECK(rt_dispatch::store_policy_of(k, 256 * MiB, 512 * MiB, 0) == RT_STORE_LARGE);
    CHECK(rt_dispatch::store_policy_of(k, 256 * MiB, 512 * MiB, 1) == RT_STORE_DEFAULT);
    CHECK(rt_dispatch::store_policy_of(k, 512 * MiB, 0, 3) == RT_STORE_LARGE);
}

// The tracker and the choice together: the bench's loops.
void loops() {
    Knobs k;
    reset_targets();
    // one context, one 256 MiB buffer: default for ever
    for (int i = 0; i < 12; ++i)
        CHECK(rt_dispatch::store_policy_of(k, 256 * MiB, track_target(0, at(1024), 256 * MiB), 2) ==
              RT_STORE_DEFAULT);
    // two slots: the first render of the first buffer sees itself alone, every later one both
    reset_targets();
    for (int i = 0; i < 12; ++i) {
        const int64_t ws = track_target(0, at(i & 1 ? 2048 : 1024), 256 * MiB);
        CHECK(rt_dispatch::store_policy_of(k, 256 * MiB, ws, 2) ==
              (i == 0 ? RT_STORE_DEFAULT : RT_STORE_LARGE));
    }
}

}  // namespace

int main() {
    same_buffer_counts_once();
    two_buffers_sum();
    entries_age_out();
    overlaps_count_once();
    devices_are_separate();
    two_threads();
    choice();
    loops();
    reset_targets();
    if (failures) return 1;
    std::printf("store policy check ok\n");
    return 0;
}
