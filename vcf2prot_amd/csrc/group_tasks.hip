// group_tasks.hip -- steps 4a and 4b on the device (include/v2p_frontend.h part 6): every (haplotype, transcript) group of the CSR
// v2p_decode_groups left on the device becomes its Instructions and then its Tasks, a lane per output transcript.
//
// The logic is host/instructions.cpp and host/transcript_tasks.cpp function by function (same citations: instruction.rs,
// transcript_instructions.rs), written as passes over the group's members: an Instruction is never stored, it is recomputed from the
// tables whenever a rule looks at it (ins_at).  Arithmetic is uint64_t and wraps where the host's does.
//
// Two launches, as the decode and the grouping do: COUNT writes {transcripts, Tasks, alt bytes, arena bytes} per item and what the
// reference aborts on; exclusive scans follow; EMIT recomputes every item and writes its Tasks, alt bytes and table rows in place.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "group_tasks.h"
#include "block_scan.hpp"

namespace v2p {
namespace {

enum : uint32_t {          // Constants.rs:3-8, same order
    MisSense, SMisSense, FrameShift, SFrameShift, InframeInsertion, SInframeInsertion, InframeDeletion, SInframeDeletion,
    StopGained, StopLost, SMisSenseAndInframeAltering, SFrameShiftAndStopRetained, SStopGainedAndInframeAltering,
    FrameShiftAndStopRetained, InframeDeletionAndStopRetained, InframeInsertionAndStopRetained, StopGainedAndInframeAltering,
    StartLost, SStopGained, StopLostAndFrameShift, MissenseAndInframeAltering, StartLostAndSpliceRegion
};
enum : uint32_t { Seq = 0, End = 1, NotSeq = 2 };          // MutatedString (mutation_ds.rs:50-76)

constexpr uint32_t FLAG_INSPECT_INS_GEN = 1u, FLAG_PANIC_INSPECT_ERR = 2u;      // include/v2p_step4a.h
constexpr int RC_OK = 0, RC_SKIP = 1, RC_PANIC = 2;                             // V2P_4A_*
constexpr char PANIC = '!';                                                    // an Instruction code that stands for `throw Panic{}`

struct Mut {
    uint32_t type, ref_len, mut_len, ref_kind, mut_kind;
    uint64_t ref_pos, mut_pos, mut_off;
    // Sequence -> every character, EndSequence -> all but the last (data.remove(data.len()-1))
    __device__ uint64_t mut_chars() const { return mut_kind == Seq ? mut_len : uint64_t(mut_len) - 1; }
    __device__ uint64_t ref_chars() const { return ref_kind == Seq ? ref_len : uint64_t(ref_len) - 1; }
};

struct Ins { char code; bool s_state; uint64_t pos_ref, pos_res, len, data, data_len; };      // data: offset in the aa bytes
struct Tk { uint32_t code; uint64_t start_pos, length, start_pos_res; };

__device__ Ins make(char code, bool s, uint64_t pos_ref, uint64_t pos_res, uint64_t len, uint64_t data, uint64_t data_len)
{
    return Ins{code, s, pos_ref, pos_res, len, data, data_len};
}
__device__ Ins phi() { return make('E', false, 0, 0, 0, 0, 0); }                               // generate_phi_instruction
__device__ Ins panic() { return make(PANIC, false, 0, 0, 0, 0, 0); }
__device__ Ins stop_gained(const Mut& m) { return make('G', false, m.ref_pos, m.mut_pos, 0, 0, 0); }
__device__ Ins stop_lost(const Mut& m)
{
    if (m.mut_kind == NotSeq) return panic();
    return make('L', false, m.ref_pos, m.mut_pos, m.mut_chars(), m.mut_off, m.mut_chars());
}
__device__ Ins frameshift(const Mut& m)
{
    if (m.mut_kind == NotSeq) return phi();
    return make('F', false, m.ref_pos, m.mut_pos, m.mut_chars(), m.mut_off, m.mut_chars());
}
__device__ Ins missense(const Mut& m)
{
    if (m.mut_kind == NotSeq) return panic();
    return make('M', false, m.ref_pos, m.mut_pos, 1, m.mut_off, m.mut_chars());
}
// the '2' / '3' branch of insertion, deletion and missense&inframe_altering; positions are taken crosswise there.  on_mut / on_ref:
// what a NotSeq mut_aa / ref_aa becomes -- 0 a panic, 1 stop_gained / stop_lost
__device__ Ins block_substitution(const Mut& m, int on_mut, int on_ref)
{
    const uint64_t pos_res = m.ref_pos, pos_ref = m.mut_pos;
    if (m.mut_kind == NotSeq) return on_mut ? stop_gained(m) : panic();
    const uint64_t nd = m.mut_chars();
    if (m.ref_kind == NotSeq) return on_ref ? stop_lost(m) : panic();
    const uint64_t nr = m.ref_chars();
    if (nd != nr) return make('3', false, pos_ref, pos_res, nr, m.mut_off, nd);
    return make('2', false, pos_ref, pos_res, nd, m.mut_off, nd);
}
__device__ Ins inframe_insertion(const Mut& m)
{
    if (m.ref_kind == Seq) { if (m.ref_len != 1) return block_substitution(m, 1, 1); }
    else if (m.ref_kind == End) return frameshift(m);
    else return panic();
    if (m.mut_kind == End) return frameshift(m);
    if (m.mut_kind == NotSeq) return stop_gained(m);
    return make('I', false, m.ref_pos, m.mut_pos, m.mut_len, m.mut_off, m.mut_len);
}
__device__ Ins inframe_deletion(const Mut& m)
{
    if (m.ref_kind == NotSeq) return stop_gained(m);
    const uint64_t len = m.ref_chars();
    uint64_t nd = 0;
    if (m.mut_kind == Seq) {
        if (m.mut_len == 1) nd = 1;
        else return block_substitution(m, 0, 0);
    } else if (m.mut_kind == End) {
        nd = uint64_t(m.mut_len) - 1;
        if (nd != 1) return frameshift(m);
    } else return stop_gained(m);
    return make('D', false, m.ref_pos, m.mut_pos, len - nd, m.mut_off, nd);
}
__device__ Ins s_frameshift(const Mut& m, bool ok)
{
    if (!ok) return phi();
    if (m.mut_kind == NotSeq) return stop_gained(m);
    Ins i = frameshift(m);
    i.code = 'R'; i.s_state = true;
    return i;
}
__device__ Ins recode(Ins i, char code) { if (i.code != 'E' && i.code != PANIC) i.code = code; return i; }
__device__ Ins starred(Ins i, char code) { if (i.code != PANIC) { i.code = code; i.s_state = true; } return i; }

// one group: members[0, n) of the CSR, read through the tables
struct Group {
    const TasksArgs& a;
    const uint32_t* members;
    uint64_t n;

    __device__ bool load(uint64_t k, Mut& m) const
    {
        const uint32_t id = members[k];
        if (id >= a.n_csq) return false;
        const StatsRec r = a.rec[id];
        const TaskAa t = a.aa[id];
        m.type = r.flags >> 8 & 0xffu;
        m.mut_pos = r.pos & 0xffffu; m.ref_pos = r.pos >> 16;
        m.ref_len = t.ref_len & TASK_AA_LEN_MASK; m.mut_len = t.mut_len & TASK_AA_LEN_MASK;
        m.ref_kind = t.ref_len >> 30; m.mut_kind = t.mut_len >> 30;
        m.mut_off = t.begin + m.ref_len;
        return true;
    }
    __device__ uint32_t pos_of(uint64_t k) const { const uint32_t id = members[k]; return id < a.n_csq ? a.rec[id].pos : 0u; }

    // instruction.rs validate_s_state: Mutation's PartialEq compares mut_aa_position only (mutation_ds.rs:174-180); the scan is over
    // mutations, those that became phi included
    __device__ bool validate_s_state(uint64_t self) const
    {
        const uint32_t mine = pos_of(self) & 0xffffu;
        uint64_t index = 0;
        while ((pos_of(index) & 0xffffu) != mine) ++index;
        for (uint64_t k = 0; k < index; ++k) {
            Mut m;
            if (!load(k, m)) continue;
            if (m.type == StopGained || m.type == FrameShift || m.type == SStopGained) return false;
            if ((m.type == InframeInsertion || m.type == InframeDeletion) && (m.mut_kind == NotSeq || m.mut_kind == End)) return false;
        }
        return true;
    }

    // Instruction::from_mutation of member k (v2p_transcript_instructions' loop body, :205-206)
    __device__ Ins ins_at(uint64_t k) const
    {
        Mut m;
        if (!load(k, m)) return panic();
        if (m.type > StartLostAndSpliceRegion || !m.ref_len || !m.mut_len) return panic();
        const bool is_s = m.type == SMisSense || m.type == SFrameShift || m.type == SInframeInsertion || m.type == SInframeDeletion ||
                          m.type == SStopGained || m.type == SMisSenseAndInframeAltering || m.type == SFrameShiftAndStopRetained ||
                          m.type == SStopGainedAndInframeAltering;
        const bool valid = is_s ? validate_s_state(k) : true;
        switch (m.type) {
            case MisSense: return missense(m);
            case SMisSense: return valid ? starred(missense(m), 'N') : phi();
            case FrameShift: return frameshift(m);
            case SFrameShift: return s_frameshift(m, valid);
            case InframeInsertion: return inframe_insertion(m);
            case SInframeInsertion: {
                if (!valid) return phi();
                const Ins i = inframe_insertion(m);
                return i.code == 'I' ? starred(i, 'J') : i;
            }
            case InframeDeletion: return inframe_deletion(m);
            case SInframeDeletion: return valid ? starred(inframe_deletion(m), 'C') : phi();          // 'C' whatever the inner call returned
            case StartLost: return make('0', false, 0, 0, 0, 0, 0);
            case StopLost: return stop_lost(m);
            case StopGained: return stop_gained(m);
            case SStopGained: return valid ? starred(stop_gained(m), 'X') : phi();
            case SMisSenseAndInframeAltering: return recode(s_frameshift(m, valid), 'K');
            case SFrameShiftAndStopRetained:
                if (m.mut_kind == NotSeq) return valid ? make('Q', true, m.ref_pos, m.mut_pos, 0, 0, 0) : phi();
                return s_frameshift(m, valid);
            case SStopGainedAndInframeAltering: return recode(valid ? starred(stop_gained(m), 'X') : phi(), 'A');
            case FrameShiftAndStopRetained: return recode(frameshift(m), 'B');
            case InframeDeletionAndStopRetained: {
                Ins i = stop_gained(m);
                i.code = 'P';
                if (m.ref_kind == End) i.len = uint64_t(m.ref_len) - 1;
                return i;
            }
            case InframeInsertionAndStopRetained: return phi();
            case StopGainedAndInframeAltering: return recode(stop_gained(m), 'T');
            case StopLostAndFrameShift: return m.ref_kind == NotSeq ? stop_lost(m) : frameshift(m);
            case MissenseAndInframeAltering:
                if (m.mut_kind == NotSeq) return recode(frameshift(m), 'Y');
                return block_substitution(m, 0, 0);
            default: return make('U', false, 0, 0, 0, 0, 0);                                          // StartLostAndSpliceRegion
        }
    }

    // #[derive(PartialEq)] on Instruction: code, s_state, pos_ref, pos_res, len, data
    __device__ bool equal(const Ins& x, const Ins& y) const
    {
        if (x.code != y.code || x.s_state != y.s_state || x.pos_ref != y.pos_ref || x.pos_res != y.pos_res || x.len != y.len || x.data_len != y.data_len) return false;
        if (x.data == y.data) return true;
        for (uint64_t i = 0; i < x.data_len; ++i) if (a.aa_bytes[x.data + i] != a.aa_bytes[y.data + i]) return false;
        return true;
    }
    // an Instruction's pos_ref is its mutation's ref or mut position, or 0 ('0', 'U'): can member k's Instruction start at pos_ref?
    __device__ bool may_start_at(uint64_t k, uint64_t pos_ref) const
    {
        const uint32_t p = pos_of(k);
        return pos_ref == 0 || (p & 0xffffu) == pos_ref || (p >> 16) == pos_ref;
    }
    // iter().position(|i| i == x) in member space: the first member whose Instruction equals x, the Instruction of member k
    __device__ uint64_t position(const Ins& x, uint64_t k) const
    {
        for (uint64_t q = 0; q < k; ++q) if (may_start_at(q, x.pos_ref) && equal(ins_at(q), x)) return q;
        return k;
    }
    // any 'G' / 'F' among the Instructions of members [0, k)
    __device__ bool gf_before(uint64_t k) const
    {
        for (uint64_t q = 0; q < k; ++q) { const char c = ins_at(q).code; if (c == 'G' || c == 'F') return true; }
        return false;
    }
    // the first member from k on that has an Instruction ('E' is dropped, transcript_instructions.rs:46-50); n if none
    __device__ uint64_t next_ins(uint64_t k, Ins& out) const
    {
        for (; k < n; ++k) { out = ins_at(k); if (out.code != 'E') return k; }
        return n;
    }
};

__device__ bool in_set(char c, const char* set) { for (; *set; ++set) if (*set == c) return true; return false; }

// where a transcript's Tasks and alt bytes go: counted always, stored by EMIT inside the arrays' sizes
template <bool EMIT>
struct Sink {
    const TasksArgs& a;
    uint64_t task_at, alt_at;            // (EMIT) the transcript's first Task and alt byte in the stream's arrays
    uint64_t n_tasks = 0, n_alt = 0;
    Tk last{2, 0, 0, 0};
    bool contiguous = true;              // INSPECT_TXP (transcript_instructions.rs:386-421)
    uint64_t counter = 0;

    __device__ void push(const Tk& t)
    {
        if (t.code == 2) return;
        if (n_tasks && t.start_pos_res != last.start_pos_res + last.length) contiguous = false;
        counter += t.length;
        if (EMIT) {
            const uint64_t at = task_at + n_tasks;
            if (at < a.out_tasks) {          // narrowed as the host's stream narrows them
                a.code[at] = uint8_t(t.code); a.start_pos[at] = uint32_t(t.start_pos); a.length[at] = uint32_t(t.length); a.start_pos_res[at] = uint32_t(t.start_pos_res);
            }
        }
        last = t;
        ++n_tasks;
    }
    __device__ void append(uint64_t data, uint64_t data_len)
    {
        if (EMIT) for (uint64_t i = 0; i < data_len; ++i) { const uint64_t at = alt_at + n_alt + i; if (at < a.out_alt) a.alt[at] = a.aa_bytes[data + i]; }
        n_alt += data_len;
    }
};

#define PHI Tk{2, 0, 0, 0}          /* a Task that is not pushed */

// transcript_instructions.rs:713-736
__device__ Tk build_base_instruction(const Ins& i, uint64_t ref_len)
{
    switch (i.code) {
        case 'Z': case 'Y': return Tk{0, 0, i.pos_ref + 1, 0};
        case 'L':
            if (i.pos_ref + 1 == ref_len) return Tk{0, 0, i.pos_ref + 1, 0};
            if (i.pos_ref == ref_len) return Tk{0, 0, i.pos_ref, 0};
            return Tk{0, 0, i.pos_res, 0};
        default: return Tk{0, 0, i.pos_ref, 0};
    }
}

constexpr int B_OK = 0, B_MUST_BE_LAST = 1, B_UNSUPPORTED = 2, B_ARITHMETIC = 3;      // V2P_4B_*
#define CHK_SUB(x, y) do { if ((x) < (y)) return B_ARITHMETIC; } while (0)   /* usize underflow panics in a debug build */

// :508-629; nx = all[position(ins) + 1]
__device__ int add_till_next_ins(const Ins& ins, const Ins& nx, const Tk& last, uint64_t ref_len, Tk* out)
{
    const uint64_t at = last.start_pos_res + last.length;
    switch (ins.code) {
        case 'D': case 'C': {
            if (nx.pos_ref == ins.pos_ref) { *out = PHI; return B_OK; }
            if (ins.pos_ref + ins.len == nx.pos_ref) { *out = PHI; return B_OK; }
            const uint64_t start = ins.pos_ref + ins.len + 1;
            if (nx.code == 'L' && nx.pos_ref + 1 == ref_len && start == nx.pos_ref) { *out = Tk{0, start, 1, at}; return B_OK; }   // :524-529
            CHK_SUB(nx.pos_ref, start);
            *out = Tk{0, start, nx.pos_ref - start, at};
            return B_OK;
        }
        case '2': case '3': {
            if (nx.pos_ref == ins.pos_ref) { *out = PHI; return B_OK; }
            if (ins.pos_ref + ins.len == nx.pos_ref) { *out = PHI; return B_OK; }
            const uint64_t start = ins.pos_ref + ins.len;
            CHK_SUB(nx.pos_ref, start);
            *out = Tk{0, start, nx.pos_ref - start, at};
            return B_OK;
        }
        default: {
            if (nx.pos_ref == ins.pos_ref) { *out = PHI; return B_OK; }
            if (nx.code == 'L' && nx.pos_ref + 1 == ref_len) {                                 // :595-602
                CHK_SUB(nx.pos_ref, ins.pos_ref);
                *out = Tk{0, ins.pos_ref + 1, nx.pos_ref - ins.pos_ref, at};
                return B_OK;
            }
            CHK_SUB(nx.pos_ref, ins.pos_ref + 1);
            *out = Tk{0, ins.pos_ref + 1, nx.pos_ref - 1 - ins.pos_ref, at};
            return B_OK;
        }
    }
}

// :633-651
__device__ int add_last_instruction(uint64_t ref_len, const Ins& i, uint64_t at, Tk* out)
{
    switch (i.code) {
        case 'D': case 'C':
            CHK_SUB(ref_len, i.pos_ref + i.len + 1);
            *out = Tk{0, i.pos_ref + i.len + 1, ref_len - i.pos_ref - i.len - 1, at};
            return B_OK;
        case '2': case '3':
            CHK_SUB(ref_len, i.pos_ref + i.len);
            *out = Tk{0, i.pos_ref + i.len, ref_len - i.pos_ref - i.len, at};
            return B_OK;
        default:
            CHK_SUB(ref_len, i.pos_ref + 1);
            *out = Tk{0, i.pos_ref + 1, ref_len - i.pos_ref - 1, at};
            return B_OK;
    }
}

// what step 4a leaves of a group for step 4b
struct Step4a { int rc; uint64_t k; Ins first, last; uint64_t first_at; bool empty; };

// v2p_transcript_instructions (transcript_instructions.rs:33-160) without the list
__device__ Step4a step4a(const Group& g, uint32_t flags)
{
    Step4a r{RC_OK, 0, phi(), phi(), 0, false};
    const bool inspect = flags & FLAG_INSPECT_INS_GEN;
    bool start_lost = false, duplicate = false, overlap = false;
    Ins prev = phi();
    for (uint64_t i = 0; i < g.n; ++i) {
        const Ins ins = g.ins_at(i);
        if (ins.code == PANIC) { r.rc = RC_PANIC; return r; }
        if (ins.code == 'E') continue;                                       // :46-50
        if (inspect) {
            // :62-82: two Instructions with one start
            for (uint64_t q = 0; q < i && !duplicate; ++q)
                if (g.may_start_at(q, ins.pos_ref)) { const Ins o = g.ins_at(q); duplicate = o.code != 'E' && o.pos_ref == ins.pos_ref; }
            if (r.k) {
                if (ins.pos_res <= prev.pos_res + prev.data_len - 1) overlap = true;                                     // :99 (usize arithmetic wraps in a release build)
                if ((prev.code == 'C' || prev.code == 'D') && ins.pos_ref <= prev.pos_res + prev.len - 1) overlap = true;     // :119-121
            }
        }
        if (!r.k) { r.first = ins; r.first_at = i; }
        start_lost |= ins.code == '0';
        r.empty |= ins.code == '0' || ins.code == 'U';
        prev = ins;
        ++r.k;
    }
    r.last = prev;
    if (!r.k) { r.rc = RC_SKIP; return r; }                                  // :52-55
    const int trouble = (flags & FLAG_PANIC_INSPECT_ERR) ? RC_PANIC : RC_SKIP;
    if (inspect && (duplicate || (r.k > 1 && !start_lost && overlap))) r.rc = trouble;
    return r;
}

// v2p_transcript_g_rep (get_g_rep :335-427, to_task :452-505, compute_expected_results_array_size :214-321) in one pass over the
// Instructions, each with the one behind it at hand
template <bool EMIT>
__device__ int step4b(const Group& g, const Step4a& s, uint64_t ref_len, Sink<EMIT>& sink, uint64_t* res_len)
{
    *res_len = 0;
    if (s.empty) return B_OK;                                                // :338-343
    sink.push(build_base_instruction(s.first, ref_len));                     // :353
    long long e = 0;
    const long long R = (long long)ref_len;
    bool gf_seen = false;                                                    // a 'G' or 'F' among the Instructions before this one
    Ins ins = s.first, nx = phi();
    uint64_t at_member = s.first_at;
    while (at_member < g.n) {
        const uint64_t nx_member = g.next_ins(at_member + 1, nx);
        const uint64_t pos = g.position(ins, at_member);                     // first-equal semantics: duplicates exist without the INSPECT checks
        const uint64_t at = sink.last.start_pos_res + sink.last.length;
        Tk it = PHI;
        switch (ins.code) {
            case 'M': case 'N':                                              // get_task_from_missense :654-663
                sink.append(ins.data, ins.data_len); sink.append(ins.data, ins.data_len);
                it = Tk{1, sink.n_alt - ins.data_len, 1, at};
                break;
            case 'F': case 'R': case 'K': case 'B': case 'Y':                // get_task_from_frameshift :666-679
                sink.append(ins.data, ins.data_len);
                it = Tk{1, sink.n_alt - ins.data_len, ins.len, at};
                break;
            case 'G': case 'X': case 'A': case 'T':                          // stop gained family: phi (:682-693)
            case 'Q': case 'Z': case 'P':                                    // :471
                break;
            case 'L': case 'W':                                              // get_task_from_stop_lost :696-710
                sink.append(ins.data, ins.data_len);
                it = Tk{1, sink.n_alt - ins.data_len, ins.data_len, at};
                break;
            case 'I': case 'J': { const uint64_t b = sink.n_alt; sink.append(ins.data, ins.data_len); it = Tk{1, b, ins.len, at}; break; }            // :739-747
            case 'D': case 'C': { const uint64_t b = sink.n_alt; sink.append(ins.data, ins.data_len); it = Tk{1, b, ins.data_len, at}; break; }       // :750-758
            case '2': { const uint64_t b = sink.n_alt; sink.append(ins.data, ins.data_len); it = Tk{1, b, ins.len, at}; break; }                      // :761-769
            case '3': { const uint64_t b = sink.n_alt; sink.append(ins.data, ins.data_len); it = Tk{1, b, ins.data_len, at}; break; }                 // :772-780
            default: return B_UNSUPPORTED;                                   // :479 panic
        }
        Tk t2 = PHI;
        if (g.equal(s.last, ins)) {                                          // :481
            if (!in_set(ins.code, "KYQABPZTWGFRLX")) {                       // :486-490
                const int rc = add_last_instruction(ref_len, ins, it.start_pos_res + it.length, &t2);      // :491
                if (rc != B_OK) return rc;
            }
        } else {
            if (in_set(ins.code, "KQABPZTWGFRL")) return B_MUST_BE_LAST;     // :496-499
            Ins after = nx;
            uint64_t after_member = nx_member;
            if (pos != at_member) after_member = g.next_ins(pos + 1, after);
            if (after_member >= g.n) return B_UNSUPPORTED;
            const int rc = add_till_next_ins(ins, after, it, ref_len, &t2);  // :500
            if (rc != B_OK) return rc;
        }
        sink.push(it);
        sink.push(t2);
        // :214-321, this Instruction's share
        const bool gf = pos == at_member ? gf_seen : g.gf_before(pos);
        const long long p = (long long)ins.pos_ref, dl = (long long)ins.data_len, ln = (long long)ins.len;
        switch (ins.code) {
            case 'F': e += dl - (R - p); break;                                              // :222
            case 'R': if (!gf) e += dl - (R - p); break;                                     // :223-232
            case 'G': case 'X': e -= R - p; break;                                           // :233
            case 'M': case 'N': case '2': break;                                             // :234
            case 'L': if (ins.pos_ref + 1 == ref_len || ins.pos_ref == ref_len) e += dl; else e += dl - (R - p); break;   // :235-245
            case 'I': e += dl - 1; break;                                                    // :246
            case 'J': if (!gf) e += dl - 1; break;                                           // :247-256
            case 'D': e -= ln; break;                                                        // :257
            case 'C': if (!gf) e -= ln; break;                                               // :258-267
            case 'K': case 'Q': if (!gf) e += dl - (R - p); break;                           // :268-287
            case 'A': if (!gf) e -= R - p; break;                                            // :288-297
            case 'B': e -= R - p - ln; break;                                                // :298
            case 'P': e -= ln; break;                                                        // :299
            case 'Z': break;                                                                 // :300
            case 'T': e -= R - p; break;                                                     // :301
            case 'W': e += dl; break;                                                        // :302
            case 'Y': e += dl - (R - p) + 1; break;                                          // :303
            case '3': e += dl - ln; break;                                                   // :304
            default: return B_UNSUPPORTED;                                                   // :305 panic
        }
        gf_seen |= ins.code == 'G' || ins.code == 'F';
        ins = nx; at_member = nx_member;
    }
    if (R + e < 0) return B_ARITHMETIC;
    *res_len = uint64_t(R + e);
    return B_OK;
}

// an item: haplotype, the transcript's row of a.tx (negative: none) and its group (or none)
struct Item { uint32_t hap; bool has_tx, has_group; uint64_t group; TaskTx tx; };

__device__ Item item_of(const TasksArgs& a, uint64_t item)
{
    Item it{0, false, false, 0, TaskTx{-1, {0, 0}, 0, 0}};
    if (!a.slot_rank) {
        // altered only: the item is group `item`; its haplotype is the list whose groups hold it
        uint32_t lo = 0, hi = a.n_haps;                                      // the last h with hap_group_begin[h] <= item
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (a.hap_group_begin[mid] <= item) lo = mid; else hi = mid; }
        it.hap = lo; it.has_group = true; it.group = item;
        const uint32_t r = a.group_transcript[item];
        if (r < a.n_tx) { it.has_tx = true; it.tx = a.tx[r]; }
        return it;
    }
    it.hap = uint32_t(item / a.n_slots);
    const uint32_t slot = uint32_t(item % a.n_slots);
    if (slot < a.n_tx) { it.has_tx = true; it.tx = a.tx[slot]; }
    const uint32_t r = a.slot_rank[slot];
    if (r == ~0u) return it;
    uint64_t lo = a.hap_group_begin[it.hap], hi = a.hap_group_begin[it.hap + 1];      // group_transcript ascends inside a list
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (a.group_transcript[mid] < r) lo = mid + 1; else hi = mid; }
    if (lo < a.hap_group_begin[it.hap + 1] && lo < a.n_groups && a.group_transcript[lo] == r) { it.has_group = true; it.group = lo; }
    return it;
}

template <bool EMIT>
__global__ __launch_bounds__(TASKS_THREADS) void group_tasks_kernel(const TasksArgs a)
{
    const uint64_t local = uint64_t(blockIdx.x) * TASKS_THREADS + threadIdx.x;
    const uint64_t item = (EMIT ? a.i0 : 0) + local;
    if (item >= (EMIT ? a.i1 : a.n_items)) return;
    const Item it = item_of(a, item);
    const bool write_all = a.slot_rank != nullptr;
    auto abort_item = [&](uint32_t why) { atomicMin(a.status, (unsigned long long)item << 8 | why); };
    uint8_t kind = TASKS_ITEM_DROPPED;
    uint64_t res_len = 0;
    TaskCount base{0, 0, 0, 0};
    if (EMIT) {
        kind = a.kinds[item];
        if (kind == TASKS_ITEM_DROPPED) return;
        base = a.base[item] - a.first;
    }
    Sink<EMIT> sink{a, base.tasks, base.alt};
    // transcript_instructions.rs:37-41: a transcript the reference FASTA does not have is skipped
    if (it.has_tx && it.tx.proteome_off >= 0) {
        const uint64_t ref_len = it.tx.ref_len;
        bool reference_copy = !it.has_group;                                 // -a: an unaltered transcript is one copy of its reference
        if (EMIT) reference_copy = kind == TASKS_ITEM_REFERENCE;
        if (!reference_copy) {
            const uint64_t m0 = a.group_member_begin[it.group], m1 = a.group_member_begin[it.group + 1];
            if (m1 < m0 || m1 > a.n_members) { if (!EMIT) abort_item(TASKS_ABORT_RANGE); return; }
            const Group g{a, a.member_ids + m0, m1 - m0};
            const Step4a s = step4a(g, a.flags);
            if (s.rc == RC_PANIC) { if (!EMIT) abort_item(TASKS_ABORT_4A); return; }
            if (s.rc == RC_SKIP) reference_copy = true;                      // (without -a: dropped)
            else {
                const int rc = step4b<EMIT>(g, s, ref_len, sink, &res_len);
                if (rc == B_MUST_BE_LAST) reference_copy = true;             // haplotype_instruction.rs:100-104: Err -> skipped
                else if (rc != B_OK) { if (!EMIT) abort_item(rc == B_ARITHMETIC ? TASKS_ABORT_4B_ARITHMETIC : TASKS_ABORT_4B_UNSUPPORTED); return; }
                else {
                    // INSPECT_TXP travels with the QC switches (cli.rs:337-368); the empty GIR returns before the validation
                    if ((a.flags & FLAG_INSPECT_INS_GEN) && sink.n_tasks && (!sink.contiguous || sink.counter != res_len)) {
                        if (!EMIT) abort_item(TASKS_ABORT_INSPECT);
                        return;
                    }
                    kind = TASKS_ITEM_TASKS;
                }
            }
            if (!EMIT && reference_copy && !write_all) reference_copy = false;
        }
        if (reference_copy) {
            // not in the haplotype's annotation -> written as reference (personalized_genome.rs:176-183): one code-0 Task of ref_len
            sink.n_tasks = 0;                                                // (COUNT may have counted Tasks before the skip; an EMIT lane comes here with nothing stored)
            sink.push(Tk{0, 0, ref_len, 0});
            sink.n_alt = 0;
            res_len = ref_len;
            kind = TASKS_ITEM_REFERENCE;
        }
    }
    if (!EMIT) {
        const bool kept = kind != TASKS_ITEM_DROPPED;
        a.kinds[item] = kind;
        a.counts[item] = kept ? TaskCount{1, sink.n_tasks, sink.n_alt, uint64_t(uint32_t(res_len)) + it.tx.header_len + (it.tx.header_len ? 1u : 0u)}
                              : TaskCount{0, 0, 0, 0};
        return;
    }
    const uint64_t t = base.tx;
    if (t < a.out_tx) {
        a.tx_proteome_off[t] = (unsigned long long)it.tx.proteome_off; a.tx_ref_len[t] = it.tx.ref_len; a.tx_res_len[t] = uint32_t(res_len);
        a.tx_task_begin[t] = base.tasks; a.tx_alt_begin[t] = base.alt;
        a.tx_header_off[t] = it.tx.header_off[it.hap & 1u]; a.tx_header_len[t] = it.tx.header_len;
    }
}

// ---- exclusive prefix sums of the items' counts: tile sums, their scan in one workgroup, the tiles again --------------------
// a tile per workgroup, TASKS_SCAN_PER_THREAD consecutive items per thread.  APPLY false: the tile's sum into block_sums[tile]; APPLY true, once
// tasks_tile_scan_kernel has turned block_sums into the tiles' bases: base[] of the tile's items
template <bool APPLY>
__global__ __launch_bounds__(TASKS_SCAN_THREADS) void tasks_tile_kernel(const TaskCount* counts, uint64_t n, TaskCount* block_sums, TaskCount* base)
{
    __shared__ TaskCount scratch[TASKS_SCAN_THREADS / 64];
    const uint64_t i0 = (uint64_t(blockIdx.x) * TASKS_SCAN_THREADS + threadIdx.x) * TASKS_SCAN_PER_THREAD;
    TaskCount s{0, 0, 0, 0}, total;
    for (uint32_t k = 0; k < TASKS_SCAN_PER_THREAD; ++k) if (i0 + k < n) s = s + counts[i0 + k];
    s = block_excl_scan<TASKS_SCAN_THREADS>(s, scratch, &total);
    if (!APPLY) { if (threadIdx.x == 0) block_sums[blockIdx.x] = total; return; }
    s = s + block_sums[blockIdx.x];
    for (uint32_t k = 0; k < TASKS_SCAN_PER_THREAD; ++k) if (i0 + k < n) { base[i0 + k] = s; s = s + counts[i0 + k]; }
}

// one workgroup, a chunk of consecutive tiles per thread; the sum of all tiles goes to *total (base[n])
__global__ __launch_bounds__(TASKS_SCAN_THREADS) void tasks_tile_scan_kernel(TaskCount* block_sums, uint64_t n_tiles, TaskCount* total)
{
    __shared__ TaskCount scratch[TASKS_SCAN_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n_tiles + TASKS_SCAN_THREADS - 1) / TASKS_SCAN_THREADS;
    const uint64_t t0 = uint64_t(tid) * per < n_tiles ? uint64_t(tid) * per : n_tiles, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    TaskCount s{0, 0, 0, 0}, all;
    for (uint64_t t = t0; t < t1; ++t) s = s + block_sums[t];
    s = block_excl_scan<TASKS_SCAN_THREADS>(s, scratch, &all);
    if (tid == 0) *total = all;
    for (uint64_t t = t0; t < t1; ++t) { const TaskCount v = block_sums[t]; block_sums[t] = s; s = s + v; }
}

__device__ uint64_t first_item(const TasksArgs& a, uint32_t h) { return a.slot_rank ? uint64_t(h) * a.n_slots : uint64_t(a.hap_group_begin[h]); }

__global__ __launch_bounds__(TASKS_SCAN_THREADS) void tasks_hap_base_kernel(const TasksArgs a)
{
    const uint64_t h = uint64_t(blockIdx.x) * TASKS_SCAN_THREADS + threadIdx.x;
    if (h > a.n_haps) return;
    const uint64_t f = first_item(a, uint32_t(h)), i = f < a.n_items ? f : a.n_items;
    a.hap_base[h] = a.base[i];
}

// EMIT's tables per haplotype and the closing entries of the two offset arrays
__global__ __launch_bounds__(TASKS_SCAN_THREADS) void tasks_hap_tables_kernel(const TasksArgs a)
{
    const uint64_t k = uint64_t(blockIdx.x) * TASKS_SCAN_THREADS + threadIdx.x;
    const uint64_t n_h = a.h1 - a.h0;
    if (k > n_h) return;
    const TaskCount b = a.hap_base[a.h0 + k];
    a.hap_tx_begin[k] = b.tx - a.first.tx;
    a.hap_out_begin[k] = b.arena - a.first.arena;
    if (k == n_h) { a.tx_task_begin[a.out_tx] = b.tasks - a.first.tasks; a.tx_alt_begin[a.out_tx] = b.alt - a.first.alt; }
}

// the routing sample (stream_item_stats): Tasks, fusable one-residue substitutions and arena bytes of every step-th transcript
__global__ __launch_bounds__(TASKS_SCAN_THREADS) void tasks_sample_kernel(const SampleArgs a)
{
    const uint64_t k = uint64_t(blockIdx.x) * TASKS_SCAN_THREADS + threadIdx.x;
    if (k >= a.n_samples) return;
    const uint64_t u = k * a.step;
    if (u >= a.n_tx) return;
    const uint64_t t0 = a.tx_task_begin[u], t1 = a.tx_task_begin[u + 1];
    uint32_t nf = 0;
    for (uint64_t i = t0 + 1; i + 1 < t1; ++i) nf += (a.code[i] == 1 && a.length[i] == 1 && a.code[i - 1] == 0 && a.code[i + 1] == 0) ? 1u : 0u;
    const uint32_t hl = a.tx_header_len ? a.tx_header_len[u] : 0u;
    a.out[k] = TaskSample{uint32_t(t1 - t0), nf, (unsigned long long)a.tx_res_len[u] + (hl ? hl + 1ull : 0ull)};
}

uint32_t blocks_for(uint64_t n, uint32_t threads) { return uint32_t((n + threads - 1) / threads); }

}  // namespace

hipError_t launch_tasks_count(const TasksArgs& a, hipStream_t st)
{
    if (!a.n_items) return hipSuccess;
    if (a.n_items > (1ull << 31) * TASKS_THREADS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_tasks_kernel<false>, dim3(blocks_for(a.n_items, TASKS_THREADS)), dim3(TASKS_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tasks_tile_scan(const TaskCount* counts, uint64_t n, TaskCount* base, TaskCount* block_sums, hipStream_t st)
{
    const uint64_t n_tiles = tasks_scan_blocks(n);
    if (n_tiles) hipLaunchKernelGGL(tasks_tile_kernel<false>, dim3(uint32_t(n_tiles)), dim3(TASKS_SCAN_THREADS), 0, st, counts, n, block_sums, base);
    hipLaunchKernelGGL(tasks_tile_scan_kernel, dim3(1), dim3(TASKS_SCAN_THREADS), 0, st, block_sums, n_tiles, base + n);
    if (n_tiles) hipLaunchKernelGGL(tasks_tile_kernel<true>, dim3(uint32_t(n_tiles)), dim3(TASKS_SCAN_THREADS), 0, st, counts, n, block_sums, base);
    return hipGetLastError();
}

hipError_t launch_tasks_scan(const TasksArgs& a, hipStream_t st)
{
    const hipError_t e = launch_tasks_tile_scan(a.counts, a.n_items, a.base, a.block_sums, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tasks_hap_base_kernel, dim3(blocks_for(uint64_t(a.n_haps) + 1, TASKS_SCAN_THREADS)), dim3(TASKS_SCAN_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tasks_emit(const TasksArgs& a, hipStream_t st)
{
    if (a.i1 > a.i0) hipLaunchKernelGGL(group_tasks_kernel<true>, dim3(blocks_for(a.i1 - a.i0, TASKS_THREADS)), dim3(TASKS_THREADS), 0, st, a);
    hipLaunchKernelGGL(tasks_hap_tables_kernel, dim3(blocks_for(uint64_t(a.h1 - a.h0) + 1, TASKS_SCAN_THREADS)), dim3(TASKS_SCAN_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tasks_sample(const SampleArgs& a, hipStream_t st)
{
    if (!a.n_samples) return hipSuccess;
    hipLaunchKernelGGL(tasks_sample_kernel, dim3(blocks_for(a.n_samples, TASKS_SCAN_THREADS)), dim3(TASKS_SCAN_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace v2p
