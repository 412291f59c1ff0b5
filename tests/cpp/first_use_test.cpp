// The first-use guard of the launch sites (rusty_compression_amd/csrc/rc_launch.hpp, rc::FirstUse) on a CPU: no HIP, no library.
//   1. eight threads share one guard over four device numbers and call it 1000 times each; the action counts per device and writes a
//      payload that every caller reads after the guard returns: each count is exactly 1 and no caller sees a missing payload
//   2. a device number of 64 or more (or below 0) runs the action on every call and never marks device 0 (or any other) done
//   3. an action that throws leaves the device unmarked: the next call runs it again, and only then is the device done
// Prints one line per check and exits non-zero when one fails.
#include <atomic>
#include <cstdio>
#include <stdexcept>
#include <thread>
#include <vector>

#include "rc_launch.hpp"

static int failures = 0;
static void expect(const char *name, long got, long want) {
    std::printf("%s %ld (want %ld)%s\n", name, got, want, got == want ? "" : "  FAILED");
    if (got != want) ++failures;
}

int main() {
    {
        constexpr int THREADS = 8, DEVICES = 4, CALLS = 1000;
        rc::FirstUse once;
        int count[DEVICES] = {};    // plain ints on purpose: the guard is all that orders the writers and the readers
        long payload[DEVICES] = {};
        std::atomic<int> ready{0};
        std::atomic<long> missing{0};
        std::vector<std::thread> pool;
        for (int t = 0; t < THREADS; ++t)
            pool.emplace_back([&, t] {
                ready.fetch_add(1);
                while (ready.load() < THREADS) std::this_thread::yield();
                for (int i = 0; i < CALLS; ++i) {
                    const int d = (t + i) % DEVICES;
                    once(d, [&] {
                        ++count[d];
                        payload[d] = 1000 + d;
                    });
                    if (payload[d] != 1000 + d) missing.fetch_add(1);
                }
            });
        for (auto &th : pool) th.join();
        for (int d = 0; d < DEVICES; ++d) expect("action runs per device", count[d], 1);
        expect("callers that saw no payload", missing.load(), 0);
    }
    {
        rc::FirstUse once;
        int runs = 0, runs0 = 0;
        for (int i = 0; i < 3; ++i) once(64, [&] { ++runs; });
        for (int i = 0; i < 3; ++i) once(128, [&] { ++runs; });
        for (int i = 0; i < 3; ++i) once(-1, [&] { ++runs; });
        expect("untracked devices run the action on every call", runs, 9);
        for (int i = 0; i < 3; ++i) once(0, [&] { ++runs0; });
        expect("device 0 after devices 64, 128 and -1", runs0, 1);
        int runs63 = 0;
        for (int i = 0; i < 3; ++i) once(63, [&] { ++runs63; });
        expect("device 63", runs63, 1);
    }
    {
        rc::FirstUse once;
        int runs = 0, caught = 0;
        try {
            once(2, [&] {
                ++runs;
                throw std::runtime_error("first use failed");
            });
        } catch (const std::runtime_error &) { ++caught; }
        expect("the throw reaches the caller", caught, 1);
        once(2, [&] { ++runs; });
        expect("the next call runs the action again", runs, 2);
        once(2, [&] { ++runs; });
        expect("and then the device is done", runs, 2);
    }
    std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
    return failures ? 1 : 0;
}
