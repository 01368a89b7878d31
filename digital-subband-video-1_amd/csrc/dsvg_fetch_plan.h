// dsvg_fetch_plan.h -- what a packet fetch (dsvg_fetch_pictures, dsvg_fetch_pictures_cb) decides on the host: plain C++17 without a HIP
// include or a context, so that a stand-alone program can compile it (tools/fetch_plan_host.cpp) and the device-free query
// dsvg_fetch_plan can ask it about any slot table and any plane sizes.  The call decides twice: plan_fetch_wait before the plane sizes
// are known (the checks, the path, the coding events to wait for and how, the copies of the one-round-trip path), plan_fetch_layout
// once they have arrived (does the round trip hold everything; else the gather table, the bytes and the pieces of the copy).
// dsvg_fetch_pictures_cb (dsvg_pipe.hip) waits, grows, copies and calls back as the two say.  A call they refuse has changed nothing.
#ifndef DSVG_FETCH_PLAN_H
#define DSVG_FETCH_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../../include/dsvg.h"

static constexpr size_t FETCH_FEW_PLANE = 65536;       // the one-round-trip path brings back this much of every plane ...
static constexpr int FETCH_FEW_MAX = 4;                // ... of at most this many pictures

// the integers of a context the decisions read: its out slots and where a slot's three payloads lie in the packed bits (CtxScan)
struct FetchGeo { int out_slots; size_t bits_per_job, bits_off[3], bits_cap[3]; };

// DSV1_NO_FETCH_FAST (A/B): read from the environment by dsvg_pipe.hip, once per process; plan_fetch_wait takes it as an argument
struct FetchSwitches { bool no_fetch_fast; };

struct FetchPlaneSize { unsigned long long total_bits; int overflow; };      // of HzPlaneSum, what the layout reads

// The coding events behind these out slots, each once, in the order they first appear: slot_ev[slot] is the event of the call that coded
// the slot last (-1: none yet).  slots == nullptr: the n slots from `first` on.
static inline void coded_events_once(const int *slot_ev, size_t nring, int n, const int *slots, int first, std::vector<int> &out)
{
    std::vector<char> seen(nring, 0);
    out.clear();
    for (int i = 0; i < n; i++) {
        const int e = slot_ev[slots ? slots[i] : first + i];
        if (e >= 0 && !seen[(size_t)e]) { seen[(size_t)e] = 1; out.push_back(e); }
    }
}

struct FetchCopy { size_t src, dst, bytes; };    // from the packed bits (bytes) to the pinned payload buffer

struct FetchWait {
    bool few;                        // the one-round-trip path
    bool stream_wait;                // the events are waited for in the fetch stream (few), else on the host
    std::vector<int> events;         // indices into the ring of coding events
    int lo, hi;                      // general (and a few path that falls through): the out slots whose plane summaries come back in one copy
    size_t grow;                     // few: elements asked of the payload pair before anything is enqueued (the `few` rule); else 0
    std::vector<FetchCopy> copy;     // few: per picture, behind the copy of its slot's three plane summaries, its three payload copies
    char err[128];                   // a refused call: the text for dsvg_last_error
};

// Before the sizes.  slot_ev: out_slots entries; slot_isP: n_isP entries (none on a context that has coded nothing: such a slot counts
// as a P picture); nring, ncalls: the ring of coding events and the coding calls made so far.  Returns DSVG_OK or the code of the first
// failed check with its text in W.err.
static inline int plan_fetch_wait(const FetchGeo &G, const FetchSwitches &sw, int n, const int *out_slots, const int *slot_ev, const char *slot_isP, size_t n_isP,
                                  size_t nring, long ncalls, int nchunks, int align, bool has_cb, FetchWait &W)
{
    W.err[0] = 0; W.few = W.stream_wait = false; W.lo = W.hi = 0; W.grow = 0; W.events.clear(); W.copy.clear();
    if (nchunks < 1 || align < 1 || !out_slots || n < 1 || n > G.out_slots) { snprintf(W.err, sizeof W.err, "bad fetch_pictures arguments"); return DSVG_ERR_ARG; }
    for (int i = 0; i < n; i++)
        if (out_slots[i] < 0 || out_slots[i] >= G.out_slots) { snprintf(W.err, sizeof W.err, "out slot out of range"); return DSVG_ERR_ARG; }
    // The frame-serial callers (ABR streams, dsv_enc without lookahead): the plane summaries and the first 64 KB of every plane's payload
    // come back in ONE round trip -- a P picture's planes are a few KB -- instead of sizes, gather table, gather kernel and payload in
    // two, and the wait can sit in the fetch stream -- but only when NOTHING else is in flight (every slot comes from the newest coding
    // call: a queued wait on a fetch stream that shares its hardware queue with a busy coding stream would stall that stream) and no
    // slot holds an I picture (their planes exceed the 64 KB the path brings back: it would pay the round trip twice).  Everyone else
    // waits ON THE HOST (the call blocks for its results anyway): later batches already enqueued keep running, and the fetch stream
    // never holds a pending wait.
    bool few = n <= FETCH_FEW_MAX && !has_cb && !sw.no_fetch_fast;
    const int newest = nring ? (int)((ncalls - 1) % (long)nring) : -1;
    for (int i = 0; i < n && few; i++) {
        const int o = out_slots[i], e = slot_ev[o];
        if (e >= 0 && e != newest) few = false;
        if ((size_t)o < n_isP && !slot_isP[o]) few = false;
    }
    W.few = W.stream_wait = few;
    W.lo = W.hi = out_slots[0];
    for (int i = 1; i < n; i++) { W.lo = std::min(W.lo, out_slots[i]); W.hi = std::max(W.hi, out_slots[i]); }
    coded_events_once(slot_ev, nring, n, out_slots, 0, W.events);
    if (!few) return DSVG_OK;
    W.grow = FETCH_FEW_MAX * 3 * FETCH_FEW_PLANE + 64;
    W.copy.resize(3 * (size_t)n);
    for (int i = 0; i < n; i++)
        for (int p = 0; p < 3; p++)
            W.copy[3 * (size_t)i + p] = { (size_t)out_slots[i] * G.bits_per_job + G.bits_off[p], (3 * (size_t)i + p) * FETCH_FEW_PLANE,
                                          std::min<size_t>(FETCH_FEW_PLANE, G.bits_cap[p]) };
    return DSVG_OK;
}

struct FetchPiece { int first, end; size_t o0, o1; };      // pictures [first, end) of the call, bytes [o0, o1) of the gathered payloads

struct FetchLayout {
    bool fits;                       // few: every plane lies within what the round trip brought back
    std::vector<uint32_t> nbytes;    // per picture and plane: the payload's bytes ...
    std::vector<size_t> pay;         // ... and where it starts in the pinned payload buffer
    std::vector<unsigned long long> rows;    // general: the gather table, per picture and plane (source byte, destination byte, bytes)
    size_t total, grow;              // general: bytes gathered (every payload padded to 16); elements asked of the payload pair
    int nchunks;                     // general: the pieces of the copy
    std::vector<FetchPiece> piece;
    char err[128];
};

// After the sizes: size[3 i + p] is plane p of out_slots[i].  few: the path plan_fetch_wait chose -- a call whose planes do not fit
// (fits == false) is planned again with few == false.  nchunks, align, has_cb: the caller's pieces, each but the last ending on a
// multiple of `align` pictures; without a callback there is one.  Returns DSVG_OK or DSVG_ERR_OVERFLOW with its text in L.err, decided
// before anything else is written.
static inline int plan_fetch_layout(const FetchGeo &G, int n, const int *out_slots, const FetchPlaneSize *size, bool few, int nchunks, int align, bool has_cb,
                                    FetchLayout &L)
{
    L.err[0] = 0; L.fits = false; L.total = L.grow = 0; L.nchunks = 0;
    L.nbytes.clear(); L.pay.clear(); L.rows.clear(); L.piece.clear();
    for (int i = 0; i < n; i++)
        for (int p = 0; p < 3; p++)
            if (size[3 * (size_t)i + p].overflow) {
                snprintf(L.err, sizeof L.err, "packed plane %d of out slot %d exceeds %zu bytes", p, out_slots[i], G.bits_cap[p]);
                return DSVG_ERR_OVERFLOW;
            }
    L.nbytes.resize(3 * (size_t)n); L.pay.resize(3 * (size_t)n);
    for (size_t k = 0; k < 3 * (size_t)n; k++) L.nbytes[k] = (uint32_t)((size[k].total_bits + 7) >> 3);
    if (few) {
        L.fits = true;
        for (size_t k = 0; k < 3 * (size_t)n; k++) {
            L.fits = L.fits && (size_t)((size[k].total_bits + 7) >> 3) <= std::min<size_t>(FETCH_FEW_PLANE, G.bits_cap[k % 3]);
            L.pay[k] = k * FETCH_FEW_PLANE;
        }
        return DSVG_OK;
    }
    // every payload compacted into one buffer on the device, 16-aligned, then copied to the host in pieces
    L.rows.resize(9 * (size_t)n);
    size_t total = 0;
    for (size_t k = 0; k < 3 * (size_t)n; k++) {
        const size_t nb = (size_t)((size[k].total_bits + 7) >> 3);
        L.rows[3 * k] = (size_t)out_slots[k / 3] * G.bits_per_job + G.bits_off[k % 3];
        L.rows[3 * k + 1] = L.pay[k] = total;
        L.rows[3 * k + 2] = nb;
        total += (nb + 15) & ~(size_t)15;
    }
    L.total = total; L.grow = total + 64;
    L.nchunks = std::max(1, std::min(has_cb ? nchunks : 1, n / align));
    L.piece.resize((size_t)L.nchunks);
    for (int j = 0, first = 0; j < L.nchunks; j++) {
        const int end = j + 1 == L.nchunks ? n : (int)((long)(n / align) * (j + 1) / L.nchunks) * align;
        L.piece[(size_t)j] = { first, end, first < n ? L.pay[3 * (size_t)first] : total, end < n ? L.pay[3 * (size_t)end] : total };
        first = end;
    }
    return DSVG_OK;
}

#endif
