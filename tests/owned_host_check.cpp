// owned_host_check.cpp — the failure contract of csrc/owned.hpp on a machine without a HIP device,
// where hipMalloc, hipHostMalloc, hipEventCreateWithFlags and hipStreamCreateWithFlags all fail
// cleanly. Built with -fsanitize=address,undefined and run directly (tests/test_owned_host.py); with a
// device present the allocations succeed and the program checks the success side instead.
#include <cstdio>
#include <cstring>
#include <utility>

#include "owned.hpp"

using namespace gsgpu;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { ++failures; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

// a lazily created group as the library's are: owners made one after the other
struct Group {
    Stream s;
    Event e[2];
    DevBuf<uint32_t> buf;
    int tag = 0;
    int create(int t) {
        tag = t;
        GS_TRY(s.create());
        GS_TRY(e[0].create());
        GS_TRY(e[1].create());
        return buf.grow(16, "group buffer");
    }
};

int main() {
    int ndev = 0;
    const bool device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    (void)hipGetLastError();
    const int want = device ? GS_OK : GS_ERR_NOMEM;

    {   // destroying and resetting empty owners is a no-op
        DevBuf<> d;
        Pinned<char> p;
        Event e;
        Stream s;
        d.reset();
        p.reset();
        e.reset();
        s.reset();
        CHECK(!d && !p && !e && !s && d.capacity() == 0);
    }
    {   // a failed grow: GS_ERR_NOMEM, pointer and capacity empty, the error set; the next tries again
        DevBuf<uint64_t> d;
        last_error().clear();
        CHECK(d.grow(1000, "first try") == want);
        CHECK(device || (d.get() == nullptr && d.capacity() == 0));
        CHECK(device || std::strstr(last_error().c_str(), "first try: 8000 bytes") != nullptr);
        last_error().clear();
        CHECK(d.grow(2000, "second try", nullptr) == want);            // (draining the null stream)
        CHECK(device || std::strstr(last_error().c_str(), "second try: 16000 bytes") != nullptr);
        CHECK(device ? (d.get() != nullptr && d.capacity() == 2000) : (d.get() == nullptr && d.capacity() == 0));
        CHECK(d.grow(0, "nothing") == GS_OK || !device);               // enough room: nothing to do
        Pinned<unsigned long long> p;
        CHECK(p.alloc(3, "pinned") == want);
        CHECK(device ? p.get() != nullptr : p.get() == nullptr);
        Event e;
        Stream s;
        CHECK((e.create() == GS_OK) == device && (e.get() != nullptr) == device);
        CHECK((s.create() == GS_OK) == device && (s.get() != nullptr) == device);
    }
    {   // moving leaves the source empty (a stand-in address: never dereferenced, released before it
        // could be freed)
        struct Fake : DevBuf<uint32_t> {
            void adopt(uint32_t* p) { this->p_ = p; }
            uint32_t* release() { return std::exchange(this->p_, nullptr); }
        };
        static uint32_t word;
        Fake a;
        a.adopt(&word);
        Fake b(std::move(a));
        CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == &word);
        Fake c;
        c = std::move(b);
        CHECK(b.get() == nullptr && c.get() == &word);
        c = std::move(c);                                               // self-move keeps it
        CHECK(c.get() == &word);
        CHECK(c.release() == &word && !c);
    }
    {   // a group whose creation fails leaves its destination untouched
        Group dst;
        dst.tag = 7;
        const int rc = make_whole(dst, 9);
        if (device) {
            CHECK(rc == GS_OK && dst.tag == 9 && dst.s && dst.e[0] && dst.e[1] && dst.buf.capacity() == 16);
        } else {
            CHECK(rc == GS_ERR_HIP);                                    // the stream, its first member
            CHECK(dst.tag == 7 && !dst.s && !dst.e[0] && !dst.e[1] && !dst.buf);
        }
    }
    if (failures) return 1;
    std::printf("owned_host_check OK (%s)\n", device ? "device present" : "no device");
    return 0;
}
