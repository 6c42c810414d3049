// resources_driver.cpp -- drives the owners of csrc/ufm_resources.h over a backend that counts: malloc / free, the live allocations per
// kind, a log of every backend call, and "fail the k-th allocation".  One printed line per case; tests/test_resources.py builds it with
// sanitizers, runs it and compares the lines with a table.  Stand-alone: it includes that header only.  The last case builds a struct
// shaped like the engine the way engine_create does and fails every one of its allocations in turn.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>

using ResStream = int *;
using ResEvent = int *;
#include "ufm_resources.h"

namespace {

constexpr int FAILED = -12;                  // what the backend answers for an allocation that fails (UFM_ERR_NOMEM)

struct Backend {
    std::set<void *> live[3], ever;          // by kind: device, pinned, event; everything ever handed out
    std::vector<std::string> log;
    int allocs = 0, frees = 0, fail_at = -1; // allocations so far (failed ones included); the one to fail, counted from 0
    int freed_twice = 0, freed_unknown = 0;
    size_t last_bytes = 0;
    Pin last_kind = Pin::Default;
    int alive() const { return (int)(live[0].size() + live[1].size() + live[2].size()); }
    std::string joined() const {
        std::string s;
        for (const std::string &l : log) s += (s.empty() ? "" : ",") + l;
        return s.empty() ? "-" : s;
    }
    int get(int kind, const char *what, void **p, size_t bytes) {
        *p = nullptr;
        char text[64];
        if (kind == 2) std::snprintf(text, sizeof(text), "%s", what);
        else std::snprintf(text, sizeof(text), "%s(%zu)", what, bytes);
        if (allocs++ == fail_at) { log.push_back(std::string(text) + "!"); return FAILED; }
        log.push_back(text);
        void *q = std::aligned_alloc(64, (bytes + 63) / 64 * 64 + 64);
        std::memset(q, 0xAA, bytes);         // (memory as it comes: not zero)
        live[kind].insert(q); ever.insert(q);
        *p = q;
        return 0;
    }
    void give(int kind, const char *what, void *p) {
        log.push_back(what);
        ++frees;
        if (!live[kind].erase(p)) { ++(ever.count(p) ? freed_twice : freed_unknown); return; }
        std::free(p);
    }
} B;

void fresh(int fail_at = -1) { B = Backend{}; B.fail_at = fail_at; }
const char *pin_name(Pin k) { return k == Pin::Default ? "default" : (k == Pin::Mapped ? "mapped" : "coherent"); }

}  // namespace

int res_dev_alloc(void **p, size_t bytes) { return B.get(0, "dev_alloc", p, bytes); }
void res_dev_free(void *p) { B.give(0, "dev_free", p); }
int res_pin_alloc(void **p, size_t bytes, Pin kind) { B.last_bytes = bytes; B.last_kind = kind; return B.get(1, (std::string("pin_alloc_") + pin_name(kind)).c_str(), p, bytes); }
void res_pin_free(void *p) { B.give(1, "pin_free", p); }
int res_event_create(ResEvent *e) { void *q; const int rc = B.get(2, "ev_create", &q, 4); *e = static_cast<int *>(q); return rc; }
void res_event_destroy(ResEvent e) { B.give(2, "ev_destroy", e); }
int res_stream_sync(ResStream) { B.log.push_back("sync"); return 0; }

namespace {

int STREAM_TOKEN = 0;
ResStream const S = &STREAM_TOKEN;

void tail() {                                // what every case ends with, once its owners are gone
    std::printf("live=%d twice=%d unknown=%d log=%s\n", B.alive(), B.freed_twice, B.freed_unknown, B.joined().c_str());
}

void fixed_arrays() {
    fresh();
    { DevArray<int> a; const int rc = a.alloc(10); std::printf("fixed_device: rc=%d held=%d ", rc, a ? 1 : 0); }
    tail();
    fresh();
    { PinArray<float> a; const int rc = a.alloc(3, Pin::Mapped); a[2] = 1.0f; std::printf("fixed_pinned: rc=%d ", rc); }
    tail();
    fresh();
    {
        DevArray<int> target;
        {
            DevArray<int> source;
            source.alloc(4);
            int *held = source;
            target = std::move(source);
            std::printf("fixed_moved_from: source_null=%d target_has_it=%d ", source ? 0 : 1, held == target ? 1 : 0);
        }
        std::printf("frees_after_source=%d ", B.frees);
    }
    tail();
    fresh();
    {
        DevArray<int> a, b;
        a.alloc(1); b.alloc(2);
        a = std::move(b);                    // what a held is given back, b's is kept
        DevArray<int> c(std::move(a));
        std::printf("fixed_move_over_held: frees_after_moves=%d a_null=%d b_null=%d ", B.frees, a ? 0 : 1, b ? 0 : 1);
    }
    tail();
    fresh();
    { DevArray<int> a; a.ensure(5); a.ensure(50); a.alloc(6); std::printf("fixed_ensure_then_alloc: "); }
    tail();
}

void grow_arrays() {
    fresh();
    { GrowArray<int> g; const int rc = g.reserve(S, 100); std::printf("grow_first: rc=%d cap=%zu ", rc, g.cap); B.log.push_back("end"); }
    tail();
    fresh();
    { GrowArray<int> g; g.reserve(S, 100, false, true); std::printf("grow_first_always_sync: cap=%zu ", g.cap); B.log.push_back("end"); }
    tail();
    fresh();
    {
        GrowArray<int> g;
        g.reserve(S, 0);                     // nothing asked of an empty one: nothing made
        const size_t cap0 = g.cap;
        g.reserve(S, 100);
        B.log.clear();
        const int *held = g;
        g.reserve(S, 100); g.reserve(S, 99); g.reserve(S, 0); g.reserve(S, 100, true, true);
        std::printf("grow_smaller_or_equal: cap_of_empty=%zu cap=%zu same_buffer=%d calls=%s ", cap0, g.cap, held == g ? 1 : 0, B.joined().c_str());
    }
    tail();
    fresh();
    { GrowArray<int> g; g.reserve(S, 100); g.reserve(S, 200); std::printf("grow_larger: cap=%zu ", g.cap); B.log.push_back("end"); }
    tail();
    fresh();
    {
        GrowArray<uint8_t, 4096> g;
        g.reserve(S, 10);
        const size_t c1 = g.cap;
        g.reserve(S, 4096);
        const size_t c2 = g.cap;
        g.reserve(S, 5000);
        std::printf("grow_floor: cap=%zu,%zu,%zu ", c1, c2, g.cap);
        B.log.push_back("end");
    }
    tail();
    fresh();
    { GrowArray<double> g; g.reserve(S, 7); std::printf("grow_elements: cap=%zu ", g.cap); B.log.push_back("end"); }
    tail();
    fresh();
    { GrowArray<int> g; g.reserve(S, 8, true); g.pinned[7] = 1; g.reserve(S, 16, true); std::printf("grow_twin_larger: cap=%zu ", g.cap); B.log.push_back("end"); }
    tail();
    fresh(1);
    {
        GrowArray<int> g;
        g.reserve(S, 100);
        const int rc = g.reserve(S, 200);
        std::printf("grow_fails: rc=%d cap=%zu null=%d frees=%d ", rc, g.cap, g.dev || g.pinned ? 0 : 1, B.frees);
        const int rc2 = g.reserve(S, 50);
        std::printf("later: rc=%d cap=%zu held=%d ", rc2, g.cap, g.dev ? 1 : 0);
        B.log.push_back("end");
    }
    tail();
    fresh(1);
    {
        GrowArray<int> g;
        const int rc = g.reserve(S, 64, true);
        std::printf("grow_twin_pinned_fails: rc=%d cap=%zu null=%d ", rc, g.cap, g.dev || g.pinned ? 0 : 1);
        B.log.push_back("end");
    }
    tail();
    fresh();
    {
        GrowArray<int> a;
        a.reserve(S, 10);
        GrowArray<int> b(std::move(a));
        std::printf("grow_moved_from: source_cap=%zu source_null=%d target_cap=%zu ", a.cap, a.dev ? 0 : 1, b.cap);
    }
    tail();
}

void event_sets() {
    fresh();
    { EventSet<2> e; std::printf("events_never_ensured: first_null=%d ", e[0] ? 0 : 1); }
    tail();
    fresh();
    { EventSet<2> e; const int r1 = e.ensure(), r2 = e.ensure(); std::printf("events_ensured_twice: rc=%d,%d both=%d ", r1, r2, e[0] && e[1] ? 1 : 0); B.log.push_back("end"); }
    tail();
    fresh(1);
    { EventSet<2> e; const int rc = e.ensure(); std::printf("events_second_create_fails: rc=%d first=%d second=%d ", rc, e[0] ? 1 : 0, e[1] ? 1 : 0); B.log.push_back("end"); }
    tail();
    fresh();
    {
        std::vector<EventSet<1>> v;
        for (int i = 0; i < 5; ++i) { EventSet<1> a; a.ensure(); v.push_back(std::move(a)); }     // (the vector grows: the sets move)
        std::printf("events_in_a_vector: destroyed_while_growing=%d ", B.frees);
    }
    std::printf("destroyed=%d ", B.frees);
    B.log.clear();
    tail();
}

struct Payload { int v[25]; };               // 100 bytes: the flag belongs at 128
void published_block() {
    fresh();
    {
        Published<Payload> pub;
        const int rc = pub.alloc();
        const Payload *data = pub;
        const uintptr_t at = reinterpret_cast<uintptr_t>(pub.flag()), from = reinterpret_cast<uintptr_t>(data);
        bool zero = *pub.flag() == 0u;
        for (int v : pub->v) zero = zero && v == 0;
        std::printf("published: rc=%d flag_aligned=%d flag_behind_payload=%d flag_at=%zu bytes=%zu kind=%s zeroed=%d ", rc, at % 64 == 0 ? 1 : 0,
                    at >= from + sizeof(Payload) ? 1 : 0, (size_t)(at - from), B.last_bytes, pin_name(B.last_kind), zero ? 1 : 0);
    }
    tail();
    fresh();
    { Published<int[2]> pub; pub.alloc(); std::printf("published_small: flag_at=%zu bytes=%zu ", (size_t)(reinterpret_cast<char *>(pub.flag()) - reinterpret_cast<char *>(pub.mem.p)), B.last_bytes); }
    tail();
}

struct Params { float *g; uint8_t *cost; int *list; int n; };      // a plain struct of pointers, as the kernels take it
std::vector<DevRow> rows_of(Params &P) { return {dev_row(P.g, 400, Fill::Inf), dev_row(P.cost, 100), dev_row(P.list, 0, Fill::Zero)}; }
void table() {
    fresh();
    {
        Params P{};
        DevTable t;
        const int rc = t.alloc(rows_of(P));
        std::printf("table: rc=%d filled=%d ", rc, P.g && P.cost && P.list ? 1 : 0);
        t.release();
        std::printf("nulled=%d ", !P.g && !P.cost && !P.list ? 1 : 0);
        t.release();
    }
    tail();
    fresh(1);
    {
        Params P{};
        DevTable t;
        const int rc = t.alloc(rows_of(P));
        std::printf("table_second_fails: rc=%d first_only=%d ", rc, P.g && !P.cost && !P.list ? 1 : 0);
        t.release(); t.release();
        std::printf("nulled=%d ", !P.g && !P.cost && !P.list ? 1 : 0);
        B.log.push_back("end");
    }
    tail();
}

// ---- a struct shaped like the engine: the stream first, then owners of every kind ----
struct Stream {
    ResStream s = nullptr;
    ~Stream() { if (s) B.log.push_back("stream_release"); }
};
struct Aggregate {
    Stream stream;
    ~Aggregate() { B.log.push_back("wait_and_drop_graphs"); }
    Params P{};
    DevTable bufs;
    Published<Payload> ctr, pipe[2];
    PinArray<int> job;
    PinArray<unsigned long long> scratch;
    EventSet<2> own_ev;
    std::vector<EventSet<1>> batch_ev;
    GrowArray<float> field;
    GrowArray<int> path;
    GrowArray<uint8_t, 4096> patch;
    DevArray<uint8_t> raw, survey[2];
    DevArray<uint32_t> census;
    Published<int[2]> range;
    PinArray<int32_t> centres;
};
#define TRY(expr) do { const int rc_ = (expr); if (rc_ != 0) return rc_; } while (0)
int aggregate_create(Aggregate **out) {
    std::unique_ptr<Aggregate> a(new Aggregate());
    a->stream.s = S;
    B.log.push_back("stream_create");
    for (Published<Payload> *p : {&a->ctr, &a->pipe[0], &a->pipe[1]}) TRY(p->alloc());
    TRY(a->job.alloc(1, Pin::Coherent));
    TRY(a->scratch.alloc(2 + 6));
    TRY(a->bufs.alloc(rows_of(a->P)));
    TRY(a->raw.alloc(100));
    for (auto &s : a->survey) TRY(s.ensure(100));
    TRY(a->own_ev.ensure());
    for (int i = 0; i < 3; ++i) { EventSet<1> e; TRY(e.ensure()); a->batch_ev.push_back(std::move(e)); }
    TRY(a->field.reserve(S, 10));
    TRY(a->field.reserve(S, 20));
    TRY(a->path.reserve(S, 10, true, true));
    TRY(a->patch.reserve(S, 9, true));
    TRY(a->census.alloc(256));
    TRY(a->range.alloc());
    TRY(a->centres.ensure(3, Pin::Mapped));
    *out = a.release();
    return 0;
}
// what must hold once the struct is gone: nothing live, nothing freed twice or unasked, the stream given back behind everything else
bool clean() {
    size_t last_free = 0, stream_at = 0;
    for (size_t i = 0; i < B.log.size(); ++i) {
        if (B.log[i].find("_free") != std::string::npos || B.log[i] == "ev_destroy") last_free = i;
        if (B.log[i] == "stream_release") stream_at = i;
    }
    return B.alive() == 0 && B.freed_twice == 0 && B.freed_unknown == 0 && stream_at > last_free && stream_at + 1 == B.log.size();
}
void aggregate() {
    fresh();
    Aggregate *whole = nullptr;
    const int rc0 = aggregate_create(&whole);
    const int total = B.allocs, live_whole = B.alive();
    delete whole;
    const bool whole_clean = clean();
    int failed = 0, failed_clean = 0;
    std::string bad;
    for (int k = 0; k < total; ++k) {
        fresh(k);
        Aggregate *a = nullptr;
        const int rc = aggregate_create(&a);
        if (rc == FAILED && !a) ++failed;
        if (clean()) ++failed_clean; else bad += (bad.empty() ? "" : ",") + std::to_string(k);
    }
    std::printf("aggregate: rc=%d allocations=%d live_when_whole=%d clean_after_delete=%d failed=%d clean_after_failure=%d not_clean=%s\n", rc0, total, live_whole,
                whole_clean ? 1 : 0, failed, failed_clean, bad.empty() ? "-" : bad.c_str());
}

}  // namespace

int main() {
    fixed_arrays();
    grow_arrays();
    event_sets();
    published_block();
    table();
    aggregate();
    return 0;
}
