// The streamed pipeline's slot protocol (vcf2prot_amd/csrc/pipe_slots.hpp) played by plain threads: 8 submitters, one runner, one thread
// that reserves, 2 slots.  Every slot field below is a plain variable, written and read only by whoever the board says owns the slot -- so
// ThreadSanitizer reports any hand-off that does not happen-before through the board, and the CHECKs catch a slot with two owners or a
// FREE slot with work left on its (simulated) streams.  Built and run by tests/test_pipe_slots.py; exit status 0 = the protocol held.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "pipe_slots.hpp"

using pipe_slots::Board;
using pipe_slots::State;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "pipe_slots_stress.cpp:%d: CHECK(%s) failed\n", __LINE__, #cond); std::_Exit(1); } } while (0)

namespace {

constexpr uint32_t N_SLOTS = 2, N_SUBMITTERS = 8, N_SUBMISSIONS = 200;
constexpr int NOBODY = -1, RUNNER = 100, RESERVE = 101;

struct Slot {                 // what PipeSlot is to the pipeline: all plain
    int owner = NOBODY;
    uint64_t staged = 0;      // the submitter's sequence number (its slice in the staging buffer)
    uint64_t result = 0;      // ... as the runner brought it home
    bool failed = false;      // the runner's rc
    int pending = 0;          // work on the slot's streams that nobody has synchronised with
    uint64_t cap = 0;         // the buffers' size: reserve's to change, a submitter's to read
    uint64_t cap_seen = 0;
};

Slot slots[N_SLOTS];

void own(uint32_t t, int who) { CHECK(slots[t].owner == NOBODY); slots[t].owner = who; }
void disown(uint32_t t, int who) { CHECK(slots[t].owner == who); slots[t].owner = NOBODY; }

bool runner_fails(uint64_t seq) { return seq % 8 == 3; }                 // one submission in eight

uint64_t run_jobs(Board& board)         // the runner: returns how many jobs it finished
{
    uint64_t n = 0;
    uint32_t t;
    while (board.take(&t)) {
        own(t, RUNNER);
        Slot& s = slots[t];
        CHECK(s.staged != 0 && s.pending == 1);
        s.failed = runner_fails(s.staged);
        s.result = s.failed ? 0 : s.staged;
        s.pending = 2;                                   // (failed or not: the streams hold its work)
        disown(t, RUNNER);
        board.finish(t, !s.failed);
        ++n;
    }
    return n;
}

void stage(uint32_t t, int who, uint64_t seq)
{
    own(t, who);
    Slot& s = slots[t];
    CHECK(s.pending == 0);                               // a FREE slot's streams are idle
    s.staged = seq;
    s.cap_seen = s.cap;                                  // (reads what reserve resizes)
    s.result = 0;
    s.pending = 1;                                       // the H2D
}

void submitter(Board& board, int id, std::atomic<uint64_t>& n_enqueued)
{
    for (uint32_t i = 0; i < N_SUBMISSIONS; ++i) {
        const uint64_t seq = uint64_t(id) * 1000000 + i + 1;
        uint32_t t;
        while (!board.claim_first_free(&t)) std::this_thread::yield();          // V2P_BUSY
        stage(t, id, seq);
        Slot& s = slots[t];
        if (seq % 16 == 9) {                             // a submission that fails half way: drained, then free again
            s.pending = 0;
            disown(t, id);
            board.unclaim(t);
            continue;
        }
        disown(t, id);
        board.enqueue(t);
        ++n_enqueued;
        const bool wait = (seq / 3) % 8 != 5;            // one in eight is released without a wait (some of them failed)
        if (wait) {
            const State st = board.settled(t);
            CHECK(st == State::LAUNCHED || st == State::FAILED);
            own(t, id);
            CHECK(s.failed == runner_fails(seq) && (st == State::FAILED) == s.failed);
            if (st == State::LAUNCHED) {
                s.pending = 0;                           // the `done` event
                CHECK(s.result == seq);
                board.ready(t);
                CHECK(board.settled(t) == State::READY && board.peek(t) == State::READY && s.result == seq);     // a second wait, result_info
            }
            disown(t, id);
        }
        // release, waited for or not
        const State st = board.settled(t);
        CHECK(st == State::LAUNCHED || st == State::FAILED || st == State::READY);
        CHECK(wait ? st != State::LAUNCHED : st != State::READY);
        own(t, id);
        if (st != State::READY) s.pending = 0;           // the event, or both streams
        CHECK(s.pending == 0 && s.staged == seq);
        disown(t, id);
        board.release(t);
    }
}

void reserver(Board& board, const std::atomic<bool>& done, uint64_t& n_reserved)
{
    while (!done.load()) {
        if (board.claim_all()) {
            for (uint32_t t = 0; t < N_SLOTS; ++t) { own(t, RESERVE); CHECK(slots[t].pending == 0); ++slots[t].cap; disown(t, RESERVE); }
            board.unclaim_all();
            ++n_reserved;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

}  // namespace

int main()
{
    Board board(N_SLOTS);
    CHECK(board.settled(0) == State::FREE && board.peek(1) == State::FREE);     // "nothing submitted on this ticket"
    std::atomic<uint64_t> n_enqueued{0};
    std::atomic<bool> done{false};
    uint64_t n_finished = 0, n_reserved = 0;
    std::thread runner([&] { n_finished = run_jobs(board); });
    std::thread res(reserver, std::ref(board), std::cref(done), std::ref(n_reserved));
    std::vector<std::thread> subs;
    for (uint32_t id = 0; id < N_SUBMITTERS; ++id) subs.emplace_back(submitter, std::ref(board), int(id), std::ref(n_enqueued));
    for (std::thread& th : subs) th.join();
    done = true;
    res.join();
    // a packed image takes slot `next` and no other
    uint32_t t, t2;
    CHECK(board.claim_next(&t));
    CHECK(!board.claim_next(&t2));
    stage(t, 0, 1); slots[t].pending = 2; disown(t, 0);
    board.launch(t);
    CHECK(board.settled(t) == State::LAUNCHED);
    CHECK(board.claim_next(&t2) && t2 == (t + 1) % N_SLOTS);
    board.unclaim(t2);
    CHECK(!board.claim_all());
    own(t, 0); slots[t].pending = 0; disown(t, 0);
    board.release(t);
    // the stop comes while jobs are queued (here: perhaps; below: certainly) -- they are still finished
    for (uint32_t k = 0; k < N_SLOTS; ++k) {
        CHECK(board.claim_first_free(&t));
        stage(t, 0, 2 * k + 10);                         // (none the runner fails)
        disown(t, 0);
        board.enqueue(t);
        ++n_enqueued;
    }
    board.stop();
    runner.join();
    CHECK(n_finished == n_enqueued.load());
    for (t = 0; t < N_SLOTS; ++t) { CHECK(board.settled(t) == State::LAUNCHED && slots[t].result == slots[t].staged); slots[t] = Slot(); }

    Board late(N_SLOTS);                                 // nobody runs yet: both jobs are queued when the stop comes
    for (uint32_t k = 0; k < N_SLOTS; ++k) {
        CHECK(late.claim_first_free(&t) && t == k);
        stage(t, 0, 2 * k + 10);
        disown(t, 0);
        late.enqueue(t);
    }
    CHECK(!late.claim_first_free(&t));
    late.stop();
    uint64_t n_late = 0;
    std::thread late_runner([&] { n_late = run_jobs(late); });
    late_runner.join();
    CHECK(n_late == N_SLOTS);
    for (t = 0; t < N_SLOTS; ++t) CHECK(late.settled(t) == State::LAUNCHED && slots[t].result == slots[t].staged);
    std::printf("ok: %llu submissions finished, %llu reserves\n", (unsigned long long)n_finished, (unsigned long long)n_reserved);
    return 0;
}
