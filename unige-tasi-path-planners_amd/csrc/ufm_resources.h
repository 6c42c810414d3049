// ufm_resources.h -- who owns the engine's memory and events: move-only owners whose destructors give back what they hold, so that a
// handle that fails half way through its creation, or is destroyed, frees everything by the order of its members alone.
// Plain C++17 without HIP: tests/cpp/resources_driver.cpp compiles this header alone, over a backend that counts.  Whoever includes it
// names the two handle types first -- ResStream and ResEvent, null when empty -- and defines the backend declared below.  The functions
// that can fail return a code of include/ufm.h, 0 (UFM_OK) for success, and leave their output null otherwise.  DESIGN.md section 5.2.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

enum class Pin { Default, Mapped, Coherent };      // pinned host memory: plain; mapped into the device; mapped and host-coherent

int res_dev_alloc(void **p, size_t bytes);
void res_dev_free(void *p);
int res_pin_alloc(void **p, size_t bytes, Pin kind);
void res_pin_free(void *p);
int res_event_create(ResEvent *e);
void res_event_destroy(ResEvent e);
int res_stream_sync(ResStream s);

// One owned pointer, given back through Free.  It converts to T *: launch sites and struct fields take it as the pointer it holds.
template <class T, void (*Free)(void *)> struct Owner {
    T *p = nullptr;
    Owner() = default;
    Owner(Owner &&o) noexcept : p(o.p) { o.p = nullptr; }
    Owner &operator=(Owner &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~Owner() { reset(); }
    void reset() { if (p) Free(p); p = nullptr; }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};
// A fixed array of n elements of T on the device / in pinned host memory.  alloc() replaces what is held, ensure() allocates once.
template <class T> struct DevArray : Owner<T, res_dev_free> {
    int alloc(size_t n) { this->reset(); return res_dev_alloc(reinterpret_cast<void **>(&this->p), n * sizeof(T)); }
    int ensure(size_t n) { return this->p ? 0 : alloc(n); }
};
template <class T> struct PinArray : Owner<T, res_pin_free> {
    int alloc(size_t n, Pin kind = Pin::Default) { this->reset(); return res_pin_alloc(reinterpret_cast<void **>(&this->p), n * sizeof(T), kind); }
    int ensure(size_t n, Pin kind = Pin::Default) { return this->p ? 0 : alloc(n, kind); }
};

// A grow-only device array of `cap` elements of T, never fewer than FLOOR once there are any, with a pinned twin of the same size if
// asked.  reserve() is one comparison when there is room.  A buffer that grows is a new one: the stream is waited for if there is
// something to free (always_sync: in any case) before it is freed; cap is 0 and both pointers null until the new allocation has succeeded.
template <class T, size_t FLOOR = 0> struct GrowArray {
    DevArray<T> dev;
    PinArray<T> pinned;
    size_t cap = 0;
    GrowArray() = default;
    GrowArray(GrowArray &&o) noexcept : dev(std::move(o.dev)), pinned(std::move(o.pinned)), cap(o.cap) { o.cap = 0; }
    int reserve(ResStream s, size_t n, bool twin = false, bool always_sync = false) { return n <= cap ? 0 : grow(s, std::max(n, FLOOR), twin, always_sync); }
    int grow(ResStream s, size_t n, bool twin, bool always_sync) {
        cap = 0;
        if (always_sync || dev || pinned) { const int rc = res_stream_sync(s); if (rc != 0) return rc; }
        pinned.reset();
        int rc = dev.alloc(n);
        if (rc == 0 && twin) rc = pinned.alloc(n);
        if (rc != 0) { dev.reset(); return rc; }
        cap = n;
        return 0;
    }
    void release() { dev.reset(); pinned.reset(); cap = 0; }     // (the caller has waited for the stream)
    operator T *() const { return dev; }
};

// N events, created on first use by ensure(); those that exist are destroyed with the set.
template <int N> struct EventSet {
    ResEvent ev[N] = {};
    EventSet() = default;
    EventSet(EventSet &&o) noexcept { for (int i = 0; i < N; ++i) { ev[i] = o.ev[i]; o.ev[i] = ResEvent{}; } }
    ~EventSet() { for (ResEvent e : ev) if (e) res_event_destroy(e); }
    int ensure() {
        for (ResEvent &e : ev) if (!e) { const int rc = res_event_create(&e); if (rc != 0) return rc; }
        return 0;
    }
    ResEvent operator[](int i) const { return ev[i]; }
};

// The published block: a payload T that a kernel writes and the host reads, and behind it, at the next 64-byte boundary, the sequence
// number of the copy the payload holds -- one mapped, host-coherent allocation, zeroed.
template <class T> struct Published {
    static constexpr size_t FLAG_AT = (sizeof(T) + 63) / 64 * 64;
    PinArray<unsigned char> mem;
    int alloc() {
        const int rc = mem.alloc(FLAG_AT + 64, Pin::Coherent);
        if (rc == 0) std::memset(mem.p, 0, FLAG_AT + 64);
        return rc;
    }
    void reset() { mem.reset(); }
    unsigned int *flag() const { return reinterpret_cast<unsigned int *>(mem.p + FLAG_AT); }
    operator T *() const { return reinterpret_cast<T *>(mem.p); }
    T *operator->() const { return *this; }
};

// A table of device arrays whose pointers live in a plain struct of somebody else's (DevParams, which the kernels take by value): one
// row per array -- the field, its size, its first contents, which the includer's code writes.  alloc() fills the fields in table order
// and stops at the first failure; release() frees what alloc() got and nulls those fields: safe after half an alloc(), and twice.
enum class Fill { None, Zero, Ones, Inf, BpNone };     // nothing; bytes 0; bytes 0xFF; floats +inf; back-pointer bytes BP_NONE
struct DevRow { void **field; size_t bytes; Fill fill; };
template <class Q> DevRow dev_row(Q *&field, size_t bytes, Fill fill = Fill::None) { return DevRow{reinterpret_cast<void **>(&field), bytes, fill}; }
struct DevTable {
    std::vector<void **> held;
    DevTable() = default;
    DevTable(DevTable &&o) noexcept : held(std::move(o.held)) { o.held.clear(); }
    ~DevTable() { release(); }
    int alloc(const std::vector<DevRow> &rows) {
        held.reserve(held.size() + rows.size());
        for (const DevRow &r : rows) {
            const int rc = res_dev_alloc(r.field, r.bytes);
            if (rc != 0) return rc;
            held.push_back(r.field);
        }
        return 0;
    }
    void release() {
        for (void **f : held) { res_dev_free(*f); *f = nullptr; }
        held.clear();
    }
};

static_assert(!std::is_copy_constructible<DevArray<int>>::value && !std::is_copy_assignable<PinArray<int>>::value &&
              !std::is_copy_constructible<GrowArray<int>>::value && !std::is_copy_constructible<EventSet<2>>::value &&
              !std::is_copy_constructible<Published<int>>::value && !std::is_copy_constructible<DevTable>::value, "owners move, they are never copied");
