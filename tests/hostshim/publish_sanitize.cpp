// publish_sanitize.cpp -- pt_publish_order.h under AddressSanitizer + UBSan as a stand-alone program (__graft_entry__.build_publish_sanitizer;
// tests/test_publish.py runs it as a child process).  Random sequences of publish / take / reader-done / pt_update_spheres / restart / forget
// over 1, 2, 3 and 8 lanes -- the events of the Python test -- against a model that keeps every outstanding read as a (lane, slot) pair.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "publish_host.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::printf("publish_sanitize: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

struct Model {
    uint32_t n_lanes, ring;
    uint64_t gen = 0, first = 1;
    std::vector<uint64_t> slot_gen;
    std::vector<std::pair<uint32_t, uint32_t>> reads;  // (lane, slot)
    bool sph_live = false;
    explicit Model(uint32_t lanes) : n_lanes(lanes), ring(lanes + 2), slot_gen(lanes + 2, 0) {}
    bool prev_intact() const { return gen >= 2 && gen - 1 >= first && slot_gen[(gen - 1) % ring] == gen - 1; }
};

void run(uint32_t n_lanes, uint32_t events)
{
    pt::PublishOrder* o = pubshim::make(n_lanes);
    Model m(n_lanes);
    CHECK(pt::publish_ring_size(n_lanes) == m.ring && m.ring <= pt::kPubMaxSlots);
    for (uint32_t e = 0; e < events; e++) {
        const uint32_t kind = rnd(16);
        if (kind < 6) {
            uint64_t out[3];
            pubshim::publish(o, (int)rnd(2), out);
            m.gen++;
            const uint32_t s = (uint32_t)(m.gen % m.ring);
            uint32_t mask = 0;
            std::vector<std::pair<uint32_t, uint32_t>> keep;
            for (const auto& r : m.reads) { if (r.second == s) mask |= 1u << r.first; else keep.push_back(r); }
            m.reads.swap(keep);
            m.slot_gen[s] = m.gen;
            m.sph_live = true;
            CHECK(out[0] == m.gen && out[1] == s && out[2] == mask);
        } else if (kind < 11) {
            const uint32_t lane = rnd(n_lanes);
            const int cur = (int)rnd(4) != 0, prev = (int)rnd(2);
            int64_t out[3];
            pubshim::take(o, lane, cur, prev, out);
            CHECK((uint64_t)out[0] == m.gen);
            if (m.gen) {
                CHECK((uint32_t)out[1] == m.gen % m.ring);
                if (cur) m.reads.push_back({ lane, (uint32_t)(m.gen % m.ring) });
                if (prev && m.prev_intact()) {
                    CHECK(out[2] == (int64_t)((m.gen - 1) % m.ring));
                    m.reads.push_back({ lane, (uint32_t)((m.gen - 1) % m.ring) });
                } else {
                    CHECK(out[2] == -1);
                }
            } else {
                CHECK(out[2] == -1);
            }
        } else if (kind < 13) {
            const uint32_t lane = rnd(n_lanes);
            pt::publish_reader_done(*o, lane);
            std::vector<std::pair<uint32_t, uint32_t>> keep;
            for (const auto& r : m.reads) if (r.first != lane) keep.push_back(r);
            m.reads.swap(keep);
        } else if (kind == 13) {
            pt::publish_host_spheres(*o);
            m.sph_live = false;
        } else if (kind == 14) {
            pt::publish_restart(*o);
            m.first = m.gen + 1;
        } else {
            pt::publish_forget(*o);
            m.first = m.gen + 1;
            m.sph_live = false;
        }
        // after every event: the header's masks are the model's outstanding reads, and the next publish writes neither the newest
        // generation's slot nor its intact predecessor's
        uint64_t st[4 + 2 * pt::kPubMaxSlots];
        pubshim::state(o, st);
        CHECK(st[0] == m.gen && st[1] == m.first && (st[2] != 0) == m.sph_live);
        for (uint32_t s = 0; s < m.ring; s++) {
            uint32_t mask = 0;
            for (const auto& r : m.reads) if (r.second == s) mask |= 1u << r.first;
            CHECK(st[4 + pt::kPubMaxSlots + s] == mask && st[4 + s] == m.slot_gen[s]);
        }
        const uint32_t next = pt::publish_slot(*o, m.gen + 1);
        if (m.gen) CHECK(next != pt::publish_slot(*o, m.gen));
        CHECK(pt::publish_prev_intact(*o, m.gen) == m.prev_intact());
        if (m.prev_intact()) CHECK(next != pt::publish_slot(*o, m.gen - 1));
    }
    delete o;
}

}  // namespace

int main()
{
    for (uint32_t lanes : { 1u, 2u, 3u, 8u })
        for (uint32_t seq = 0; seq < 600; seq++) run(lanes, 40 + rnd(80));
    std::printf("publish_sanitize ok\n");
    return 0;
}
