/* srcchain_plan_host.c -- the plans of a session's source side (csrc/host/dsv1_srcchain_plan.h) on the CPU, for a sanitizer: the walk
 * of tests/test_srcchain_plan_host.py -- breadth-first from the empty chain over every reachable state, every request at every state
 * (set, change and clear of every pass, valid and not, the resets, the seek; busy and not), every call form -- for F in {4, 6, 5}, 4:2:0
 * and 4:2:2, a session that keeps its lane and one that does not; after each plan its invariants are checked.
 *   cc -O1 -g -std=c99 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all tools/srcchain_plan_host.c -o srcchain_plan_host
 *   ./srcchain_plan_host */
#include <stdio.h>
#include <stdlib.h>
#include "../digital-subband-video-1_amd/csrc/host/dsv1_srcchain_plan.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "F %d subsamp 0x%x keep %d state %d request %d: %s (line %d)\n", F, sub, keep, head, nq, #c, __LINE__); exit(1); } } while (0)

enum { W = 64, H = 48, IN_W = 80, IN_H = 60, NSRC = 2, MAXSTATES = 1024, MAXREQ = 64 };

static int same_state(const dsv1_srcchain_state *a, const dsv1_srcchain_state *b)
{
    int p;
    for (p = 0; p < DSV1_SC_SLOTS; p++)
        if (a->kind[p] != b->kind[p]) return 0;
    return a->conv_rgb == b->conv_rgb && a->conv_fb == b->conv_fb && a->deint_mode == b->deint_mode && a->orient == b->orient &&
           a->in_w == b->in_w && a->in_h == b->in_h && a->ov_clip[0] == b->ov_clip[0] && a->ov_clip[1] == b->ov_clip[1];
}

/* every request tried at a state whose raw picture is g->w x g->h */
static int requests(const dsv1_srcchain_geom *g, dsv1_srcchain_req *q)
{
    static const int orient[4] = {0, 1, 5, 9}, reset_kind[3] = {DSV1_SC_DEINTERLACE, DSV1_SC_IVTC, DSV1_SC_DENOISE};
    int n = 0, k, i, v;
    memset(q, 0, sizeof(*q) * MAXREQ);
    for (k = DSV1_SC_CONVERT; k <= DSV1_SC_OVERLAY; k++) {
        if (k == DSV1_SC_ORIENT) {
            for (i = 0; i < 4; i++, n++) { q[n].kind = k; q[n].set = q[n].valid = 1; q[n].mode = orient[i]; }
            continue;
        }
        /* v: 0 clear, 1 set, 2 set but invalid, 3 a second setting (RGB, field rate, the identity), 4 a reframe onto another canvas */
        for (v = 0; v < 5; v++) {
            if (v == 3 && k != DSV1_SC_CONVERT && k != DSV1_SC_DEINTERLACE && k != DSV1_SC_LEVELS && k != DSV1_SC_REFRAME) continue;
            if (v == 4 && k != DSV1_SC_REFRAME) continue;
            q[n].kind = k; q[n].set = v != 0; q[n].valid = v != 2;
            q[n].mode = v == 3 && k != DSV1_SC_LEVELS;
            q[n].identity = v == 3;
            q[n].frame_bytes = v == 3 ? (size_t)3 * g->w * g->h : 2 * g->fb;
            q[n].w = v == 3 ? W : IN_W; q[n].h = v == 3 ? H : IN_H; q[n].out_w = v == 4 ? W / 2 : W; q[n].out_h = v == 4 ? H / 2 : H;
            n++;
        }
    }
    for (i = 0; i < 3; i++)
        for (v = -1; v <= NSRC; v += v < 0 ? 1 : NSRC, n++) { q[n].op = DSV1_SC_OP_RESET; q[n].kind = reset_kind[i]; q[n].source = v; }
    for (i = 0; i < 2; i++, n++) { q[n].op = DSV1_SC_OP_SEEK; q[n].kind = DSV1_SC_OVERLAY; q[n].source = i ? -2 : 1; }
    return n;
}

int main(void)
{
    static const int Fs[3] = {4, 6, 5}, subs[2] = {0x5, 0x4};
    long nstates_all = 0, ntrans_all = 0, ncalls_all = 0, seen[DSV1_SCT_ROWS] = {0};
    int fi, si, keep, row;
    for (fi = 0; fi < 3; fi++)
        for (si = 0; si < 2; si++)
            for (keep = 0; keep < 2; keep++) {
                const int F = Fs[fi], sub = subs[si];
                dsv1_srcchain_state *states = (dsv1_srcchain_state *)calloc(MAXSTATES, sizeof(*states));
                dsv1_srcchain_req *q = (dsv1_srcchain_req *)calloc(MAXREQ, sizeof(*q));
                int nstates = 1, head, nq = 0;
                if (!states || !q) return 2;
                states[0].nsrc = NSRC; states[0].F = F; states[0].subsamp = sub; states[0].keep_lane = keep; states[0].ow = W; states[0].oh = H;
                for (head = 0; head < nstates; head++) {
                    const dsv1_srcchain_state s = states[head];
                    const dsv1_srcchain_geom g = dsv1_scp_geom(&s);
                    const int total = requests(&g, q);
                    int busy, p, i, form, active, clipped, any = 0;
                    CHECK(total <= MAXREQ);
                    for (p = 0; p < DSV1_SC_SLOTS; p++) any |= s.kind[p];
                    CHECK(g.lane == (keep || any));
                    for (nq = 0; nq < total; nq++)
                        for (busy = 0; busy < 2; busy++) {
                            dsv1_srcchain_set_plan P;
                            q[nq].busy = busy;
                            CHECK(dsv1_scp_req_ok(&q[nq]));
                            P = dsv1_scp_set(&s, &q[nq]);
                            ntrans_all++;
                            CHECK(P.text >= 0 && P.text < DSV1_SCT_ROWS && dsv1_scp_text(P.text));
                            CHECK((P.rc != 0) == (P.text != 0) && (P.rc == 0 || P.rc == DSVG_ERR_ARG));
                            seen[P.text]++;
                            if (P.rc || P.noop) CHECK(same_state(&P.next, &s));            /* a refusal changes nothing */
                            for (p = 0; p < DSV1_SC_SLOTS; p++) {
                                const size_t fb = p >= DSV1_SCP_REFRAME ? P.g.ofb : p == DSV1_SCP_ORIENT ? P.g.mfb : P.g.fb;
                                if (P.rc) CHECK(!P.alloc[p] && !P.free_[p] && !P.reset[p]);
                                if (P.alloc[p]) CHECK(P.alloc[p] == fb * NSRC * (size_t)(p <= DSV1_SCP_LEVELS ? P.g.conv_frames : F) && P.next.kind[p]);
                                if (P.free_[p] && p != DSV1_SCP_OVERLAY) CHECK(s.kind[p]);
                                if (P.reset[p] && p != DSV1_SCP_OVERLAY) CHECK(s.kind[p] && (q[nq].op == DSV1_SC_OP_RESET || p != dsv1_scp_pos(q[nq].kind)));
                                if (!P.rc && !P.noop && q[nq].op == DSV1_SC_OP_SET && p != DSV1_SCP_OVERLAY) CHECK((P.alloc[p] != 0) >= (P.next.kind[p] != s.kind[p] && P.next.kind[p]));
                            }
                            CHECK(P.g.frames_in > 0 && P.g.bytes_in > 0);
                            if (P.rc) continue;
                            for (i = 0; i < nstates && !same_state(&states[i], &P.next); i++) ;
                            if (i == nstates) { CHECK(nstates < MAXSTATES); states[nstates++] = P.next; }
                        }
                    for (clipped = 0; clipped <= (s.kind[DSV1_SCP_OVERLAY] != 0); clipped++)
                        for (form = 0; form <= DSV1_CLIP_HELD; form++)
                            for (active = 0; active < 2; active++) {
                                dsv1_srcchain_state c = s;
                                dsv1_srcchain_call_plan P;
                                int cur;
                                c.ov_clip[0] = clipped;
                                P = dsv1_scp_call(&c, form, active, 0);
                                ncalls_all++;
                                CHECK((P.rc != 0) == !g.lane);
                                if (P.rc) continue;
                                CHECK(P.nsteps >= 0 && P.nsteps <= DSV1_SC_MAX_STEPS);
                                cur = P.upload ? DSV1_SC_UPLOAD : DSV1_SC_CALLER;
                                for (i = 0; i < P.nsteps; i++) {
                                    const dsv1_srcchain_step *S = &P.step[i];
                                    CHECK(S->src == cur);                               /* the previous step's destination, or the input */
                                    CHECK(S->dst != DSV1_SC_CALLER && (S->dst >= 0 || !form));  /* a caller's clip is never written */
                                    CHECK(S->dst < DSV1_SC_SLOTS && S->pos >= 0 && S->pos < DSV1_SC_SLOTS && S->nframes > 0);
                                    CHECK(S->kind == DSV1_SC_NONE ? S->bytes == g.ofb * NSRC * (size_t)F && S->alloc == (clipped ? 0 : S->bytes) : S->kind == c.kind[S->pos] && !S->alloc);
                                    cur = S->dst;
                                }
                                CHECK(P.out == cur);
                                CHECK(P.bypass == (!P.nsteps && !P.upload));            /* bypass iff nothing is enqueued */
                                CHECK(P.upload == (form || P.bypass ? 0 : g.bytes_in));
                                CHECK(P.advance == (c.kind[DSV1_SCP_OVERLAY] ? F : 0));
                            }
                }
                /* converter x levels x deinterlacer / IVTC x denoise x orientation x reframe x overlays */
                CHECK(nstates == 3 * 2 * (2 + !(F & 1) + !(F % 4)) * 2 * (sub == 0x5 ? 3 : 2) * 2 * 2);
                nstates_all += nstates;
                free(states); free(q);
            }
    for (row = 0; row < DSV1_SCT_ROWS; row++)
        if (dsv1_scp_text(row)[0] && !seen[row]) { fprintf(stderr, "refusal row %d never produced: %s\n", row, dsv1_scp_text(row)); return 1; }
    printf("srcchain_plan_host: %ld states, %ld requests, %ld calls: invariants hold, every refusal row produced\n", nstates_all, ntrans_all, ncalls_all);
    return 0;
}
