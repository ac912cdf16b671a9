// fir_shard_workers.h -- the host threads of a sharded handle that lists several devices (fir_shard.hip), and the two small
// things they hand to each other: an error text kept aside and a verdict one slot publishes for the others. Host only: nothing
// of HIP or RCCL is included, so tests/shard_workers_main.cpp builds this header alone under the thread and address sanitizers.
#pragma once
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

extern "C" const char* fir_last_error(void);               // include/fir_amd.h: this thread's message
extern "C" void fir_set_last_error_(const char* msg);      // fir_internal.h

namespace fir {

// fir_last_error()'s text kept aside while later calls overwrite it (the exchange a failed rank still enters, another thread's
// buffer): always terminated, put back with restore().
struct KeptError {
    char text[512] = "";
    void capture() {
        strncpy(text, fir_last_error(), sizeof(text) - 1);
        text[sizeof(text) - 1] = 0;
    }
    void restore() const { fir_set_last_error_(text); }
};

// What one slot of a call has to finish before the others go on (search_host: slot 0 makes sure of the staging area all of
// them read): it publishes its return code, once, whether that is a failure or not; wait() blocks until then and returns it.
struct Published {
    std::mutex mu;
    std::condition_variable cv;
    bool ready = false;
    int rc = 0;
    void publish(int r) {
        { std::lock_guard<std::mutex> lk(mu); ready = true; rc = r; }
        cv.notify_all();
    }
    int wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return ready; });
        return rc;
    }
};

struct Worker {       // one thread per device of a multi-device handle: its launches and its RCCL calls
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, done = false, quit = false;
    int rc = 0;
    KeptError err;
    void loop() {
        for (;;) {
            std::function<int()> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return has_job || quit; });
                if (quit) return;
                j = job;
                has_job = false;
            }
            const int r = j();
            {
                std::lock_guard<std::mutex> lk(mu);
                rc = r;
                if (r) err.capture();
                done = true;
            }
            cv.notify_all();
        }
    }
};

// The workers of one handle: none for a one-device handle, whose calls run on the caller's thread.
struct Workers {
    std::vector<std::unique_ptr<Worker>> w;
    Workers() = default;
    Workers(const Workers&) = delete;
    Workers& operator=(const Workers&) = delete;
    ~Workers() { stop(); }
    // one thread per slot when there are two slots or more; false: host allocation failed (what has started stays until stop())
    bool start(int slots) {
        for (int s = 0; slots > 1 && s < slots; ++s) {
            Worker* k = new (std::nothrow) Worker();
            if (!k) return false;
            w.emplace_back(k);
            k->th = std::thread([k] { k->loop(); });
        }
        return true;
    }
    void stop() {
        for (auto& k : w) {
            { std::lock_guard<std::mutex> lk(k->mu); k->quit = true; }
            k->cv.notify_all();
            if (k->th.joinable()) k->th.join();
        }
        w.clear();
    }
    // Run fn(slot) for every slot: inline for one device, on the per-device worker threads otherwise. Returns the code of the
    // lowest slot that failed, with that slot's message as the calling thread's fir_last_error().
    int run_all(const std::function<int(int)>& fn) {
        if (w.empty()) return fn(0);
        for (size_t s = 0; s < w.size(); ++s) {
            Worker* k = w[s].get();
            {
                std::lock_guard<std::mutex> lk(k->mu);
                k->job = [fn, s] { return fn((int)s); };
                k->has_job = true;
                k->done = false;
            }
            k->cv.notify_all();
        }
        int rc = 0;
        for (auto& k : w) {
            std::unique_lock<std::mutex> lk(k->mu);
            k->cv.wait(lk, [&] { return k->done; });
            if (k->rc && rc == 0) { rc = k->rc; k->err.restore(); }
        }
        return rc;
    }
};

}  // namespace fir
