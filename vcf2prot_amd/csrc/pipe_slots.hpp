// The streamed pipeline's slot board: the one place that knows a slot's life (v2p_pipeline_* in v2p_api.hip).  Plain C++17, nothing of
// HIP: tests/pipe_slots_stress.cpp plays the protocol on it under ThreadSanitizer.
//
//   state      meaning                                                                who owns the slot's other fields
//   FREE       nobody's; ITS STREAMS ARE IDLE                                         nobody
//   STAGING    claimed by a submitter (or by a reserve, which claims every slot)      that submitter
//   QUEUED     in the runner's queue                                                  the runner, once it has taken the job
//   LAUNCHED   everything is enqueued, `done` is recorded                             whoever waits or releases
//   FAILED     the runner failed: rc / err / err_index are set, the streams may       whoever waits or releases
//              hold partial work
//   READY      waited for: the result is in h_out and stays valid until release       the caller
//
//   claim  FREE -> STAGING      unclaim  STAGING -> FREE       enqueue  STAGING -> QUEUED      launch  STAGING -> LAUNCHED (packed images)
//   finish QUEUED -> LAUNCHED | FAILED        ready  LAUNCHED -> READY        release  LAUNCHED | FAILED | READY -> FREE
//
// Whoever moves a slot to FREE has drained its streams first.  A slot's fields are written and read by its owner only; ownership passes
// inside the calls below, so every hand-off (submitter -> runner -> waiter -> next submitter) happens-before through the board's mutex.
//
// LOCK RULE.  The context's mutex comes before the board's; nothing is acquired while the board's is held (no call below calls out).
// What must be reported through the context (v2p_ctx::fail) is decided here and reported after the call has returned.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

namespace pipe_slots {

enum class State : uint8_t { FREE, STAGING, QUEUED, LAUNCHED, FAILED, READY };

class Board {
public:
    explicit Board(uint32_t n_slots = 0) : st_(n_slots, State::FREE) {}

    // ---- submitters ----
    // a stream slice takes the first free slot from `next` on (one submitter that releases in order sees them round-robin; workers that
    // release as they finish take whichever is free), and the slots behind it are the next submitters'; false: every slot is in use
    bool claim_first_free(uint32_t* t)
    {
        std::lock_guard<std::mutex> lk(mu_);
        const uint32_t ns = uint32_t(st_.size());
        for (uint32_t k = 0; k < ns; ++k) {
            const uint32_t i = (next_ + k) % ns;
            if (st_[i] != State::FREE) continue;
            st_[i] = State::STAGING;
            next_ = (i + 1) % ns;
            *t = i;
            return true;
        }
        return false;
    }
    // a packed image takes slot `next` and no other (`next` moves on when it is launched); false: that slot is in use
    bool claim_next(uint32_t* t)
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (st_[next_] != State::FREE) return false;
        st_[next_] = State::STAGING;
        *t = next_;
        return true;
    }
    // every slot at once (their buffers are about to be resized); false: one is in use, none was claimed
    bool claim_all()
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (State s : st_) if (s != State::FREE) return false;
        for (State& s : st_) s = State::STAGING;
        return true;
    }
    void unclaim(uint32_t t) { set(t, State::FREE); }
    void unclaim_all() { for (uint32_t t = 0; t < st_.size(); ++t) set(t, State::FREE); }
    void enqueue(uint32_t t)
    {
        { std::lock_guard<std::mutex> lk(mu_); st_[t] = State::QUEUED; jobs_.push_back(t); }
        cv_.notify_all();
    }
    void launch(uint32_t t)
    {
        { std::lock_guard<std::mutex> lk(mu_); st_[t] = State::LAUNCHED; next_ = (t + 1) % uint32_t(st_.size()); }
        cv_.notify_all();
    }

    // ---- the runner ----
    // the next queued slot, in submission order; false: stopped, and nothing is queued (what was queued at the stop has still been
    // handed out -- its waiters are owed an answer)
    bool take(uint32_t* t)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !jobs_.empty(); });
        if (jobs_.empty()) return false;
        *t = jobs_.front();
        jobs_.erase(jobs_.begin());
        return true;
    }
    void finish(uint32_t t, bool ok) { set(t, ok ? State::LAUNCHED : State::FAILED); }
    void stop()
    {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
    }

    // ---- whoever holds the ticket ----
    // blocks while the slot is a submitter's or the runner's; then FREE, LAUNCHED, FAILED or READY
    State settled(uint32_t t)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return st_[t] != State::STAGING && st_[t] != State::QUEUED; });
        return st_[t];
    }
    State peek(uint32_t t)
    {
        std::lock_guard<std::mutex> lk(mu_);
        return st_[t];
    }
    void ready(uint32_t t) { set(t, State::READY); }
    void release(uint32_t t) { set(t, State::FREE); }

private:
    void set(uint32_t t, State s)
    {
        { std::lock_guard<std::mutex> lk(mu_); st_[t] = s; }
        cv_.notify_all();
    }

    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<State> st_;
    std::vector<uint32_t> jobs_;           // slots queued for the runner, in submission order
    uint32_t next_ = 0;
    bool stop_ = false;
};

}  // namespace pipe_slots
