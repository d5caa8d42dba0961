// v2p_ctx_internal.h -- what other translation units of libvcf2prot_hip.so may do with a v2p_ctx (defined in v2p_api.hip), and the
// owners of device memory and events they share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <string>

struct v2p_ctx;
struct v2p_stream;
struct v2p_batch;

namespace v2p {
hipStream_t ctx_stream(v2p_ctx* c);
int ctx_device(v2p_ctx* c);
int ctx_fail(v2p_ctx* c, int code, const std::string& msg, int64_t index);
void ctx_lock(v2p_ctx* c);
void ctx_unlock(v2p_ctx* c);

// A resident transcript stream (v2p_stream, include/vcf2prot_hip.h) whose arrays are written by kernels, not uploaded
// (v2p_decode_tasks_emit).  All three are called with the context locked.
struct StreamArrays {                  // device pointers into the stream's one allocation (stream_layout) and its alt bytes
    unsigned long long *hap_tx_begin, *tx_proteome_off; uint32_t *tx_ref_len, *tx_res_len; unsigned long long *tx_task_begin, *tx_alt_begin;
    uint8_t* code; uint32_t *start_pos, *length, *start_pos_res; uint8_t* alt; unsigned long long* tx_header_off; uint32_t* tx_header_len;
};
// a FASTA stream of these sizes, every byte of its allocation zero (the slack behind the Task arrays with it), enqueued on the context's stream
int stream_born_alloc(v2p_ctx* c, uint64_t n_haps, uint64_t n_tx, uint64_t n_tasks, uint64_t n_alt, v2p_stream** out, StreamArrays* arrays);
// the three host-side things of a stream: hap_out_begin[n_haps + 1] and the routing statistics {items, descriptors, arena bytes} x {mean, variance}
// (stream_item_stats); then the tile tables, as behind an upload.  Waits for the context's stream.
int stream_born_finish(v2p_ctx* c, v2p_stream* st, const uint64_t* hap_out_begin, const double* stats);
void stream_born_drop(v2p_stream* st);
// what the host checks of a transcript before a stream may name it: inside the resident proteome, its record header inside the header table
// and ending in a line feed.  Returns a V2P_ERR_* code and says why.
int ctx_check_transcript(v2p_ctx* c, uint64_t proteome_off, uint32_t ref_len, uint64_t header_off, uint32_t header_len, std::string* why);

// What the distinct-record set (unique_records.hip) reads of a batch and of a resident stream; both are called with the context locked.
struct BatchArenaView { v2p_ctx* ctx; const uint8_t* arena; uint64_t out_bytes, n_haps; const unsigned long long* hap_out_begin; bool executed, orphaned; };
struct StreamRecordView {
    v2p_ctx* ctx; uint64_t n_haps, n_tx, out_bytes;
    const unsigned long long *hap_tx_begin, *tx_proteome_off; const uint32_t *tx_ref_len, *tx_res_len, *tx_header_len;   // tx_header_len: nullptr for plain tapes
};
void batch_arena_view(const ::v2p_batch* b, BatchArenaView* v);
void stream_record_view(const ::v2p_stream* s, StreamRecordView* v);

// V2P_DEBUG_POISON=1 (a debugging aid like the reference's DEBUG_* switches; read once): every device buffer is filled with 0xA5 whenever a
// call (re)sizes it -- also when the allocation is reused -- so that nothing can lean on what fresh or recycled memory happens to hold
// (tools/fuzz_*.py and the GPU suite run clean under it; one bug of that kind was found without it)
inline bool debug_poison()
{
    static const bool on = [] { const char* e = getenv("V2P_DEBUG_POISON"); return e && e[0] == '1'; }();
    return on;
}

// One device allocation and its owner.  alloc(n) is a hipMalloc of exactly n bytes -- no slack, nothing kept for reuse -- poisoned under
// debug_poison(); whatever the owner held before is freed first.
class DevMem {
    void* p_ = nullptr;
public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevMem& operator=(DevMem&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~DevMem() { reset(); }
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc(&p_, n);
        if (e != hipSuccess) p_ = nullptr;
        else if (debug_poison() && n) { (void)hipDeviceSynchronize(); (void)hipMemset(p_, 0xA5, n); (void)hipDeviceSynchronize(); }
        return e;
    }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    template <class T> T* get() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }
};

// N events, created by create() and destroyed with their owner
template <int N> class Events {
    hipEvent_t e_[N] = {};
public:
    Events() = default;
    Events(const Events&) = delete;
    ~Events() { for (hipEvent_t x : e_) if (x) (void)hipEventDestroy(x); }
    hipError_t create() {
        for (hipEvent_t& x : e_) if (!x) { const hipError_t e = hipEventCreate(&x); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    hipEvent_t operator[](int k) const { return e_[k]; }
};
}  // namespace v2p
