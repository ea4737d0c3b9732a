// TEST INFRASTRUCTURE: the happens-before checker of the stand-in HIP layer (stub_order.hpp has the model).
#include "stub_order.hpp"

#include <map>
#include <mutex>
#include <set>

namespace stub_order {
namespace {

typedef std::map<int, unsigned long long> vclock;      // stream id -> tick
void join(vclock &a, const vclock &b)
{
    for (const auto &kv : b) { unsigned long long &t = a[kv.first]; if (kv.second > t) t = kv.second; }
}
struct access {
    int sid = 0;
    unsigned long long tick = 0, seq = 0;
    const char *op = "";
    kind k = READ;
};
bool ordered_before(const access &x, const vclock &now)
{
    const auto it = now.find(x.sid);
    return it != now.end() && it->second >= x.tick;
}
// [start (the map's key), end) of one allocation: the last writer and who read / accumulated since
struct segment {
    size_t end = 0;
    bool written = false;
    access w;
    std::vector<access> r, a;
};
struct allocation {
    size_t bytes = 0;
    std::map<size_t, segment> segs;
};
struct state {
    std::mutex m;
    bool on = false;
    int next_sid = 1;                                  // (0: the null stream; ids are never reused, handles may be)
    std::map<const void *, int> sid;
    std::map<int, const void *> handle;
    std::map<int, vclock> clock;
    std::map<const void *, vclock> event;
    vclock host;
    std::map<const char *, allocation> allocs;
    unsigned long long seq = 0;
    std::set<std::pair<unsigned long long, unsigned long long>> seen;
    std::vector<report> reports;
    std::vector<wait_entry> waits;
    namer *names = nullptr;
    int ignore_wait = -1;
};
state &S()
{
    static state s;
    return s;
}
int sid_of(state &s, const void *stream)
{
    if (!stream) return 0;
    const auto it = s.sid.find(stream);
    if (it != s.sid.end()) return it->second;
    const int id = s.next_sid++;
    s.sid[stream] = id; s.handle[id] = stream;
    return id;
}
std::string stream_name(state &s, int sid)
{
    if (sid == 0) return "the null stream";
    const auto it = s.handle.find(sid);
    std::string n = it != s.handle.end() && s.names ? s.names->stream(it->second) : std::string();
    return n.empty() ? "stream #" + std::to_string(sid) : n;
}
const char *kind_name(kind k) { return k == READ ? "reads" : k == WRITE ? "writes" : "accumulates into"; }
const char *kind_noun(kind k) { return k == READ ? "read" : k == WRITE ? "write" : "accumulate"; }

void conflict(state &s, const access &was, const access &now, const char *base, size_t offset)
{
    if (!s.seen.insert(std::make_pair(was.seq, now.seq)).second) return;      // one report per pair of operations
    report r;
    r.op_a = was.op; r.op_b = now.op; r.stream_a = stream_name(s, was.sid); r.stream_b = stream_name(s, now.sid);
    r.buffer = s.names ? s.names->buffer(base) : std::string();
    if (r.buffer.empty()) r.buffer = "caller allocation";
    r.offset = offset;
    r.text = r.op_b + " on " + r.stream_b + " " + kind_name(now.k) + " " + r.buffer + " + " + std::to_string(offset) + ", not ordered behind the " + kind_noun(was.k) +
             " of " + r.op_a + " on " + r.stream_a;
    s.reports.push_back(r);
}
// the segment that starts at `at` (splitting the one that holds it)
std::map<size_t, segment>::iterator split(allocation &al, size_t at)
{
    auto it = al.segs.upper_bound(at);
    --it;
    if (it->first == at) return it;
    segment tail = it->second;
    it->second.end = at;
    return al.segs.insert(std::make_pair(at, tail)).first;
}
void drop_ordered(std::vector<access> &v, const vclock &now)
{
    size_t k = 0;
    for (size_t i = 0; i < v.size(); i++) if (!ordered_before(v[i], now)) v[k++] = v[i];      // (what is ordered before this access is ordered before whatever follows it)
    v.resize(k);
}

}  // namespace

void enable(bool on)
{
    state &s = S();
    std::lock_guard<std::mutex> g(s.m);
    s.on = on;
    if (!on) {
        s.sid.clear(); s.handle.clear(); s.clock.clear(); s.event.clear(); s.host.clear(); s.allocs.clear(); s.seen.clear(); s.reports.clear(); s.waits.clear();
        s.ignore_wait = -1;
    }
}
bool on() { return S().on; }
void set_namer(namer *n) { S().names = n; }
void clear_log()
{
    state &s = S();
    std::lock_guard<std::mutex> g(s.m);
    s.reports.clear(); s.waits.clear(); s.seen.clear();
}
const std::vector<report> &reports() { return S().reports; }
const std::vector<wait_entry> &waits() { return S().waits; }
void ignore_wait_after(int n) { S().ignore_wait = n; }

void on_malloc(void *p, size_t n)
{
    state &s = S();
    if (!s.on || !p) return;
    std::lock_guard<std::mutex> g(s.m);
    allocation &al = s.allocs[(const char *)p];
    al.bytes = n; al.segs.clear();
    al.segs[0].end = n;
}
void on_free(void *p)
{
    state &s = S();
    if (!s.on || !p) return;
    std::lock_guard<std::mutex> g(s.m);
    for (const auto &kv : s.clock) join(s.host, kv.second);
    s.allocs.erase((const char *)p);
}
void on_stream_destroy(const void *h)
{
    state &s = S();
    if (!s.on || !h) return;
    std::lock_guard<std::mutex> g(s.m);
    const auto it = s.sid.find(h);
    if (it != s.sid.end()) { s.handle.erase(it->second); s.sid.erase(it); }
}
void on_event_destroy(const void *e)
{
    state &s = S();
    if (!s.on) return;
    std::lock_guard<std::mutex> g(s.m);
    s.event.erase(e);
}
void on_record(const void *e, const void *h)
{
    state &s = S();
    if (!s.on || !e) return;
    std::lock_guard<std::mutex> g(s.m);
    s.event[e] = s.clock[sid_of(s, h)];
}
void on_wait(const void *h, const void *e)
{
    state &s = S();
    if (!s.on || !e) return;
    std::lock_guard<std::mutex> g(s.m);
    const int sid = sid_of(s, h);
    wait_entry w;
    w.stream = stream_name(s, sid);
    w.event = s.names ? s.names->event(e) : std::string();
    if (w.event.empty()) w.event = "an event of the caller's";
    if (s.ignore_wait == 0) w.ignored = true;
    if (s.ignore_wait >= 0) s.ignore_wait--;
    s.waits.push_back(w);
    const auto it = s.event.find(e);
    if (!w.ignored && it != s.event.end()) join(s.clock[sid], it->second);
}
void host_join_stream(const void *h)
{
    state &s = S();
    if (!s.on) return;
    std::lock_guard<std::mutex> g(s.m);
    join(s.host, s.clock[sid_of(s, h)]);
}
void host_join_event(const void *e)
{
    state &s = S();
    if (!s.on) return;
    std::lock_guard<std::mutex> g(s.m);
    const auto it = s.event.find(e);
    if (it != s.event.end()) join(s.host, it->second);
}
void host_join_all()
{
    state &s = S();
    if (!s.on) return;
    std::lock_guard<std::mutex> g(s.m);
    for (const auto &kv : s.clock) join(s.host, kv.second);
}

op::op(const void *stream, const char *n) : live(false), sid(0), tick(0), seq(0), name(n)
{
    state &s = S();
    if (!s.on) return;
    std::lock_guard<std::mutex> g(s.m);
    live = true;
    sid = sid_of(s, stream);
    vclock &c = s.clock[sid];
    join(c, s.host);
    tick = ++c[sid];
    seq = ++s.seq;
}
void op::touch(kind k, const void *p, size_t bytes) const
{
    if (!live || !p || !bytes) return;
    state &s = S();
    std::lock_guard<std::mutex> g(s.m);
    auto ia = s.allocs.upper_bound((const char *)p);
    if (ia == s.allocs.begin()) return;
    --ia;
    allocation &al = ia->second;
    size_t a = (size_t)((const char *)p - ia->first);
    if (a >= al.bytes) return;                         // (host memory, a page-locked block: invisible to the layer)
    const size_t b = a + bytes < al.bytes ? a + bytes : al.bytes;
    const vclock &now = s.clock[sid];
    access me;
    me.sid = sid; me.tick = tick; me.seq = seq; me.op = name; me.k = k;
    auto it = split(al, a);
    if (b < al.bytes) { split(al, b); it = al.segs.find(a); }
    for (; it != al.segs.end() && it->first < b; ++it) {
        segment &g2 = it->second;
        const size_t off = it->first;
        if (g2.written && !ordered_before(g2.w, now)) conflict(s, g2.w, me, ia->first, off);
        if (k != READ) for (const access &x : g2.r) if (!ordered_before(x, now)) conflict(s, x, me, ia->first, off);
        if (k != ACCUM) for (const access &x : g2.a) if (!ordered_before(x, now)) conflict(s, x, me, ia->first, off);
        if (k == WRITE) { g2.written = true; g2.w = me; g2.r.clear(); g2.a.clear(); }
        else {
            std::vector<access> &v = k == READ ? g2.r : g2.a;
            drop_ordered(v, now);
            if (v.empty() || v.back().seq != seq) v.push_back(me);
        }
    }
}
void op::touch_rows(kind k, const void *p, size_t pitch, size_t width, size_t rows) const
{
    if (!live) return;
    if (pitch == width) { touch(k, p, width * rows); return; }
    for (size_t y = 0; y < rows; y++) touch(k, (const char *)p + y * pitch, width);
}

}  // namespace stub_order
