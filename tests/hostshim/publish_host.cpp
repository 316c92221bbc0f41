// publish_host.cpp -- pt_publish_order.h compiled as host C++ for tests/test_publish.py (__graft_entry__.build_publish_shim).
#include "publish_host.h"

extern "C" {

void* pub_new(uint32_t n_lanes) { return pubshim::make(n_lanes); }
void pub_free(void* o) { delete static_cast<pt::PublishOrder*>(o); }
uint32_t pub_ring_size(uint32_t n_lanes) { return pt::publish_ring_size(n_lanes); }
uint32_t pub_max_lanes(void) { return pt::kPubMaxLanes; }
uint32_t pub_max_slots(void) { return pt::kPubMaxSlots; }
uint32_t pub_slot(void* o, uint64_t g) { return pt::publish_slot(*static_cast<pt::PublishOrder*>(o), g); }
int pub_prev_intact(void* o, uint64_t g) { return pt::publish_prev_intact(*static_cast<pt::PublishOrder*>(o), g) ? 1 : 0; }
void pub_publish(void* o, int with_rotations, uint64_t* out) { pubshim::publish(static_cast<pt::PublishOrder*>(o), with_rotations, out); }
void pub_take(void* o, uint32_t lane, int want_current, int want_prev, int64_t* out) { pubshim::take(static_cast<pt::PublishOrder*>(o), lane, want_current, want_prev, out); }
void pub_reader_done(void* o, uint32_t lane) { pt::publish_reader_done(*static_cast<pt::PublishOrder*>(o), lane); }
void pub_host_spheres(void* o) { pt::publish_host_spheres(*static_cast<pt::PublishOrder*>(o)); }
void pub_host_rotations(void* o) { pt::publish_host_rotations(*static_cast<pt::PublishOrder*>(o)); }
void pub_restart(void* o) { pt::publish_restart(*static_cast<pt::PublishOrder*>(o)); }
void pub_forget(void* o) { pt::publish_forget(*static_cast<pt::PublishOrder*>(o)); }
void pub_state(void* o, uint64_t* out) { pubshim::state(static_cast<pt::PublishOrder*>(o), out); }

}  // extern "C"
