// sweep3_check — the control flow of the cover sweeps' software pipeline (pandepth_amd/csrc/pd_cover_rule.h: pdcover::sweep3, three buffers in turn,
// a loop of whole rotations with ONE exit and a tail without loads) on the CPU, with loads and work that only keep a record.
// Built with -fsanitize=address,undefined by tests/test_sweep3_order.py.  For every nq of 1 .. 10, a stop behind every chunk position 0 .. nq and no
// stop at all, buffers of 4 and of 8 words:
//   * work is called for exactly the chunks 0 .. min(nq - 1, the stop's chunk), in order
//   * work(q) receives the buffer that load(., q) filled, every word of it
//   * no buffer is loaded into between its load and its work
//   * before work(q) the loads of chunks q + 1 and q + 2 were issued, where the sweep has such chunks: two chunks in flight
//   * no load's index exceeds nq + 3 (this loop's own bound: nq + 1); the loads of chunks 0 and 1 are the first two, primed() follows them and runs once
//   * the loop with an exit behind every chunk, as the sweeps had it before (kept below as the reference), makes the same sequence of work calls
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../pandepth_amd/csrc/pd_cover_rule.h"

static int g_fail = 0;
static unsigned long g_runs = 0, g_works = 0, g_loads = 0, g_late_loads = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; if (g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

// the reference: the loop with an exit behind every rotation, as the sweeps had it
template <int N, class Load, class Work, class Stop, class Primed>
static void sweep3_reference(const Load &load, const Work &work, const uint32_t nq, const Stop &stop, const Primed &primed)
{
    uint32_t A[N], B[N], C[N];
    uint32_t q = 0;
    load(A, 0u);
    load(B, 1u);
    primed();
    for (;;) {
        load(C, q + 2u);
        work(A, q);
        if (++q >= nq || stop()) break;
        load(A, q + 2u);
        work(B, q);
        if (++q >= nq || stop()) break;
        load(B, q + 2u);
        work(C, q);
        if (++q >= nq || stop()) break;
    }
}

enum Kind { LOAD, WORK, PRIMED };
struct Event { Kind kind; const uint32_t *buf; uint32_t q; bool intact; };

// what one run did
struct Trace {
    std::vector<Event> ev;
    std::vector<uint32_t> worked() const
    {
        std::vector<uint32_t> w;
        for (const Event &e : ev) if (e.kind == WORK) w.push_back(e.q);
        return w;
    }
};

static const uint32_t NO_STOP = ~0u;

template <int N, bool REFERENCE>
static Trace run(const uint32_t nq, const uint32_t stop_at)
{
    Trace t;
    bool stopped = false;
    auto load = [&](uint32_t (&x)[N], const uint32_t q) {
        for (int k = 0; k < N; ++k) x[k] = q * 16u + (uint32_t)k;
        t.ev.push_back(Event{LOAD, &x[0], q, true});
    };
    auto work = [&](uint32_t (&x)[N], const uint32_t q) {
        bool intact = true;
        for (int k = 0; k < N; ++k) intact = intact && x[k] == q * 16u + (uint32_t)k;
        t.ev.push_back(Event{WORK, &x[0], q, intact});
        if (q == stop_at) stopped = true;                // (the kernel: the chunk's work met a gap)
    };
    auto stop = [&]() -> bool { return stopped; };
    auto primed = [&]() { t.ev.push_back(Event{PRIMED, nullptr, 0u, true}); };
    if (REFERENCE) sweep3_reference<N>(load, work, nq, stop, primed);
    else pdcover::sweep3<N>(load, work, nq, stop, primed);
    return t;
}

static void check_trace(const char *form, const int n, const Trace &t, const uint32_t nq, const uint32_t stop_at, const uint32_t max_load)
{
    const uint32_t last = stop_at < nq - 1u ? stop_at : nq - 1u;
    const std::vector<uint32_t> w = t.worked();
    CHECK(w.size() == (size_t)last + 1u, "%s<%d> nq %u stop %d: %zu chunks worked on, expected %u", form, n, nq, (int)stop_at, w.size(), last + 1u);
    for (size_t i = 0; i < w.size(); ++i) CHECK(w[i] == (uint32_t)i, "%s<%d> nq %u stop %d: work call %zu is for chunk %u", form, n, nq, (int)stop_at, i, w[i]);
    CHECK(t.ev.size() >= 3 && t.ev[0].kind == LOAD && t.ev[0].q == 0u && t.ev[1].kind == LOAD && t.ev[1].q == 1u && t.ev[2].kind == PRIMED,
          "%s<%d> nq %u: the sweep does not begin load(0), load(1), primed()", form, n, nq);
    unsigned primed = 0;
    for (size_t i = 0; i < t.ev.size(); ++i) {
        const Event &e = t.ev[i];
        if (e.kind == PRIMED) { ++primed; continue; }
        if (e.kind == LOAD) {
            ++g_loads;
            if (e.q >= nq) ++g_late_loads;
            CHECK(e.q <= nq + 3u && e.q <= max_load, "%s<%d> nq %u stop %d: load of chunk %u", form, n, nq, (int)stop_at, e.q);
            continue;
        }
        ++g_works;
        CHECK(e.intact, "%s<%d> nq %u stop %d: work(%u) got a buffer that does not hold chunk %u", form, n, nq, (int)stop_at, e.q, e.q);
        // the load of this chunk: into this buffer, and no other load into it since
        long at = -1;
        for (long j = (long)i - 1; j >= 0; --j)
            if (t.ev[(size_t)j].kind == LOAD && t.ev[(size_t)j].q == e.q) { at = j; break; }
        CHECK(at >= 0, "%s<%d> nq %u stop %d: chunk %u was never loaded", form, n, nq, (int)stop_at, e.q);
        if (at < 0) continue;
        CHECK(t.ev[(size_t)at].buf == e.buf, "%s<%d> nq %u stop %d: work(%u) got another buffer than load(%u) filled", form, n, nq, (int)stop_at, e.q, e.q);
        for (size_t j = (size_t)at + 1; j < i; ++j)
            CHECK(!(t.ev[j].kind == LOAD && t.ev[j].buf == e.buf), "%s<%d> nq %u stop %d: chunk %u loaded over chunk %u before its work", form, n, nq,
                  (int)stop_at, t.ev[j].q, e.q);
        // two chunks in flight behind the one worked on: the loads of chunks q + 1 and q + 2, where the sweep has such chunks, were issued before work(q)
        bool l1 = e.q + 1u >= nq, l2 = e.q + 2u >= nq;
        for (size_t j = 0; j < i; ++j) if (t.ev[j].kind == LOAD) { l1 = l1 || t.ev[j].q == e.q + 1u; l2 = l2 || t.ev[j].q == e.q + 2u; }
        CHECK(l1 && l2, "%s<%d> nq %u stop %d: work(%u) without the next two chunks' loads issued", form, n, nq, (int)stop_at, e.q);
    }
    CHECK(primed == 1u, "%s<%d> nq %u: primed() ran %u times", form, n, nq, primed);
}

template <int N>
static void check_all()
{
    for (uint32_t nq = 1; nq <= 10u; ++nq)
        for (uint32_t s = 0; s <= nq + 1u; ++s) {
            const uint32_t stop_at = s <= nq ? s : NO_STOP;       // behind chunk 0 .. nq - 1, behind a chunk that does not exist, never
            const Trace one = run<N, false>(nq, stop_at), ref = run<N, true>(nq, stop_at);
            check_trace("sweep3", N, one, nq, stop_at, nq + 1u);
            check_trace("reference", N, ref, nq, stop_at, nq + 1u);
            CHECK(one.worked() == ref.worked(), "<%d> nq %u stop %d: sweep3 and the reference differ in their work calls", N, nq, (int)stop_at);
            g_runs += 2;
        }
}

int main()
{
    check_all<4>();
    check_all<8>();
    printf("sweeps %lu, work calls %lu, loads %lu, of them behind the last chunk %lu\n", g_runs, g_works, g_loads, g_late_loads);
    if (g_fail) { printf("sweep3_check: %d checks FAILED\n", g_fail); return 1; }
    printf("sweep3_check: ok\n");
    return 0;
}
