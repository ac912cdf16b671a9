// The worker threads of a multi-device sharded handle (csrc/fir_shard_workers.h) on their own: a stand-alone program, built by
// tests/test_shard_workers.py under the thread sanitizer and under the address / undefined-behaviour sanitizers. No GPU, no
// library: the two error functions the header declares are the stubs below, over a thread_local buffer as the library's are.
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "fir_shard_workers.h"

static thread_local char g_err[1024] = "";
extern "C" const char* fir_last_error(void) { return g_err; }
extern "C" void fir_set_last_error_(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg ? msg : ""); }
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static const int kRounds = 3000;
static bool fails(int round, int slot) { return ((unsigned)(round * 2654435761u) >> (8 + slot)) % 4 == 0; }   // a quarter of the (round, slot) pairs
static int code_of(int slot) { return -(10 + slot); }

// every slot's job runs exactly once per round, on that slot's own thread, always the same one
static void once_per_round_on_its_own_thread(int slots) {
    fir::Workers pool;
    CHECK(pool.start(slots));
    CHECK(pool.w.size() == (slots > 1 ? (size_t)slots : 0));
    std::vector<int> runs((size_t)slots, 0);
    std::vector<std::thread::id> who((size_t)slots);
    const std::thread::id caller = std::this_thread::get_id();
    for (int r = 0; r < kRounds; ++r) {
        const int rc = pool.run_all([&](int s) -> int {
            CHECK(s >= 0 && s < slots && runs[(size_t)s] == r);
            if (r == 0) who[(size_t)s] = std::this_thread::get_id();
            CHECK(who[(size_t)s] == std::this_thread::get_id());
            runs[(size_t)s]++;
            return 0;
        });
        CHECK(rc == 0);
        for (int s = 0; s < slots; ++s) CHECK(runs[(size_t)s] == r + 1);
    }
    for (int s = 0; s < slots; ++s) {
        CHECK((who[(size_t)s] == caller) == (slots == 1));             // one device: inline, on the caller's thread
        for (int t = 0; t < s; ++t) CHECK(who[(size_t)s] != who[(size_t)t]);
    }
}

// the code of the lowest failing slot, with that slot's text of THIS round as the caller's last error
static void lowest_failing_slot_wins(int slots) {
    fir::Workers pool;
    CHECK(pool.start(slots));
    int failed_rounds = 0;
    for (int r = 0; r < kRounds; ++r) {
        fir_set_last_error_("stale");
        const int rc = pool.run_all([&](int s) -> int { return fails(r, s) ? fail(code_of(s), "round %d slot %d", r, s) : 0; });
        int lowest = -1;
        for (int s = slots - 1; s >= 0; --s)
            if (fails(r, s)) lowest = s;
        if (lowest < 0) { CHECK(rc == 0); continue; }
        ++failed_rounds;
        CHECK(rc == code_of(lowest));
        CHECK(std::string(fir_last_error()) == "round " + std::to_string(r) + " slot " + std::to_string(lowest));
    }
    CHECK(failed_rounds > kRounds / 8 && failed_rounds < kRounds);
}

// search_host's handshake: slot 0 makes something all slots read and publishes its verdict, a result or a failure; the others
// block until then. A short sleep on either side forces both orders of arrival.
static void handshake_completes_in_every_order(int slots) {
    fir::Workers pool;
    CHECK(pool.start(slots));
    for (int r = 0; r < 300; ++r) {
        fir::Published staged;
        int staging = 0;                                  // (what slot 0 prepares: read by the others after wait() only)
        const int verdict0 = r % 2 ? code_of(0) : 0;
        std::atomic<int> adopted{0};
        const int rc = pool.run_all([&](int s) -> int {
            int mine = 0;
            if ((r % 3 == 0) == (s == 0)) std::this_thread::sleep_for(std::chrono::microseconds(50));
            if (s == 0) {
                if (verdict0) mine = fail(verdict0, "round %d: no staging area", r);
                else staging = r + 1;
                staged.publish(mine);
            } else {
                const int r0 = staged.wait();
                if (!mine) mine = r0;
                CHECK(r0 == verdict0 && (r0 || staging == r + 1));
                adopted++;
            }
            return mine;
        });
        CHECK(adopted == slots - 1 && rc == verdict0);
        if (rc) CHECK(std::string(fir_last_error()) == "round " + std::to_string(r) + ": no staging area");
    }
}

// a pool goes away cleanly right after creation, after work and after a failed round
static void teardown(int slots) {
    for (int i = 0; i < 50; ++i) {
        { fir::Workers pool; CHECK(pool.start(slots)); }
        { fir::Workers pool; CHECK(pool.start(slots)); CHECK(pool.run_all([](int) { return 0; }) == 0); }
        { fir::Workers pool; CHECK(pool.start(slots)); CHECK(pool.run_all([&](int s) { return s == slots - 1 ? fail(-3, "last slot") : 0; }) == -3); }
        fir::Workers pool;
        CHECK(pool.start(slots));
        pool.stop();                                      // (what teardown_devices does; the destructor then finds nothing)
        CHECK(pool.w.empty());
    }
}

int main() {
    fir::KeptError kept;                                  // always terminated, whatever the length of the text
    fir_set_last_error_(std::string(900, 'x').c_str());
    kept.capture();
    CHECK(std::string(kept.text) == std::string(511, 'x'));
    fir_set_last_error_("short");
    kept.restore();
    CHECK(std::string(fir_last_error()) == std::string(511, 'x'));
    for (int slots : {1, 2, 8}) {
        once_per_round_on_its_own_thread(slots);
        lowest_failing_slot_wins(slots);
        handshake_completes_in_every_order(slots);
        teardown(slots);
        printf("slots %d ok\n", slots);
    }
    printf("ok\n");
    return 0;
}
