// TEST INFRASTRUCTURE (tests/test_stream_order_host.py): a happens-before checker for the stand-in HIP layer.  OFF by default - the
// stand-in then behaves as before (streams execute at once, events are always complete, a wait is a null check).  Switched on
// (tests/hoststub/order_main.cpp alone does), it keeps a vector clock per stream, one for the host and one per recorded event, and for every
// live hipMalloc allocation the byte intervals with their last writer and the readers / accumulators since.  It RECORDS conflicts and
// never prints or aborts by itself: a program reads stub_order::reports().
//
// Model
//   * an operation enqueued on stream S joins the host clock into S's clock, then ticks S;
//   * hipEventRecord(e, S) stores a copy of S's clock in e; hipStreamWaitEvent(S, e) joins it into S (never recorded: nothing, as in HIP);
//   * hipStreamSynchronize, hipEventSynchronize, a successful hipEventQuery and hipDeviceSynchronize join into the host clock;
//   * hipFree joins everything into the host clock and drops the allocation's records;
//   * a blocking hipMemcpy is an operation on the null stream followed by a host join: it does NOT order behind non-blocking streams.
// Accesses: a read must be ordered after the last overlapping write; a write after the last overlapping write and every overlapping read
// and accumulate since; an accumulate (commutative atomic update) after the last write and every read since - not after other accumulates.
// Pointers outside every live device allocation (host arrays, page-locked blocks) are ignored.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace stub_order {

enum kind { READ = 0, WRITE = 1, ACCUM = 2 };

struct report {
    std::string text;          // "<op b> on <stream b> <kind> <buffer> + <offset> unordered behind <op a> on <stream a> (<kind>)"
    std::string op_a, op_b, stream_a, stream_b, buffer;
    size_t offset = 0;
};
struct wait_entry {
    std::string stream, event;     // names at the time of the wait (the namer below)
    bool ignored = false;
};
// names of streams, events and buffers: asked for whenever a report or a wait is logged, so that handles created lazily inside the call
// that conflicts already carry their names.  Each returns "" for what it does not know (buffer: `base` is the allocation's first byte)
struct namer {
    virtual std::string stream(const void *s) = 0;
    virtual std::string event(const void *e) = 0;
    virtual std::string buffer(const void *base) = 0;
    virtual ~namer() {}
};

void enable(bool on);          // off: every hook returns at once and all state is dropped
bool on();
void set_namer(namer *n);      // (not owned; nullptr: numbers only)
void clear_log();              // forgets the reports and the wait log (clocks and access records stay)
const std::vector<report> &reports();
const std::vector<wait_entry> &waits();
void ignore_wait_after(int n); // test knob: the n-th hipStreamWaitEvent from now (0 = the next) joins nothing; the caller still sees success.  -1: off

// ---- hooks of the stand-in HIP layer (hip/hip_runtime.h, stub_kernels.cpp)
void on_malloc(void *p, size_t n);
void on_free(void *p);
void on_stream_destroy(const void *s);
void on_event_destroy(const void *e);
void on_record(const void *e, const void *s);
void on_wait(const void *s, const void *e);
void host_join_stream(const void *s);
void host_join_event(const void *e);
void host_join_all();

// ---- one operation on a stream with the device memory it touches (a launcher's stand-in, an asynchronous copy, a memset)
struct op {
    op(const void *stream, const char *name);      // joins the host clock into the stream's, ticks the stream
    void touch(kind k, const void *p, size_t bytes) const;
    void touch_rows(kind k, const void *p, size_t pitch_bytes, size_t width_bytes, size_t rows) const;   // a strided box, row by row
    void read(const void *p, size_t bytes) const { touch(READ, p, bytes); }
    void write(const void *p, size_t bytes) const { touch(WRITE, p, bytes); }
    void accum(const void *p, size_t bytes) const { touch(ACCUM, p, bytes); }
    bool live;
    int sid;
    unsigned long long tick, seq;
    const char *name;
};

}  // namespace stub_order
