// pixmap_host.cpp -- TEST SHIM: the C entry points over pixmap_host.h for tests/test_pixel_map.py.
// Not part of the product; never loaded by it.
#include "pixmap_host.h"

extern "C" {

// the pair for d: out = {mul, shift}
void pix_host_pair(uint32_t d, uint32_t* out)
{
    const pt::MagicDiv m = pt::make_magic_div(d);
    out[0] = m.mul; out[1] = m.shift;
}

uint64_t pix_host_div_range(uint32_t d, uint32_t lo, uint32_t hi, uint32_t* first_bad) { return pixhost::div_mismatches(d, lo, hi, first_bad); }

// mismatches over an explicit list of n
uint64_t pix_host_div_list(uint32_t d, uint32_t count, const uint32_t* n, uint32_t* first_bad)
{
    const pt::MagicDiv m = pt::make_magic_div(d);
    uint64_t bad = 0;
    for (uint32_t i = 0; i < count; i++)
        if (pt::magic_div(n[i], m) != n[i] / d) { if (bad++ == 0 && first_bad) *first_bad = n[i]; }
    return bad;
}

uint32_t pix_host_n_slots(const uint32_t* desc) { return pixhost::make_map(desc).n_slots; }

// the map as the kernels receive it, word by word (sizeof(PixelMap) / 4 words); returns the word count
uint32_t pix_host_map_words(const uint32_t* desc, uint32_t* out)
{
    const pt::PixelMap pm = pixhost::make_map(desc);
    if (out) __builtin_memcpy(out, &pm, sizeof pm);
    return (uint32_t)(sizeof pm / 4u);
}

void pix_host_map(const uint32_t* desc, uint32_t n, const uint32_t* slots, uint32_t* out, int form)
{
    pixhost::map_slots(pixhost::make_map(desc), n, slots, out, form);
}

}
