// SHARC.hpp -- C++ host mirror of the reference's SHARC pass object (Source/SHARC.ixx:22-57) as Raytracing::Render(..., SHARC&,
// SHARCSettings) uses it (Source/Raytracing.ixx:114-148), over pt_render_sharc (row N14, DESIGN.md spec S20), a stand-in for the SHARC
// library, which the reference does not vendor.  The reference's object owns the hash entries and the two voxel buffers; here the
// context owns them, and the object carries the capacity they are made for and whether the next frame restarts them (App.cpp:672-675).
#pragma once

#include <cstdint>

namespace dxrs {

struct SHARC {
    struct Constants {  // SHARC.ixx:23-27
        uint32_t AccumulationFrames = 10, MaxStaleFrames = 64;
        float SceneScale = 50;
        bool IsAntiFireflyEnabled{};  // the filter of row N19 (DESIGN.md spec S25): Raytracing::Render routes such a frame to pt_render_sharc_ex
    };

    // SHARC::Configure: the cache is made for `capacity` slots (a power of two) and starts empty
    void Configure(uint32_t capacity = 1u << 22) noexcept
    {
        m_capacity = capacity;
        m_reset = true;
    }

    uint32_t GetCapacity() const noexcept { return m_capacity; }

    // whether the next frame restarts the cache; Render clears it once such a frame has been queued
    bool NeedsReset() const noexcept { return m_reset; }
    void ClearReset() noexcept { m_reset = false; }

private:
    uint32_t m_capacity = 1u << 22;
    bool m_reset = true;
};

}  // namespace dxrs
