/*
 * ref_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * extern "C" entry points, shaped like the vko_* calls of ../vkt_oracle.h, that run the
 * volkit REFERENCE's compiled serial CPU code.  Built by oracle/ref/Makefile against a
 * reference checkout (its headers are only #included at build time) into
 * oracle/_ref/libvktref.so; loaded by oracle/refbinding.py.
 *
 * Every entry point builds reference StructuredVolumes, copies the caller's bytes in, calls
 * the reference (default execution policy: CPU, serial) and copies the bytes out.
 *
 * Two ops have no buildable translation unit (Fill.cpp and Resample.cpp pull in
 * HierarchicalVolumeView.hpp, which needs visionaray):
 *   - FillRange runs the reference's StructuredVolumeView::setValue over the range.
 *   - Resample restates the two branches of reference src/vkt/Resample_serial.hpp: the
 *     same-dims branch (:32-48) through StructuredVolume::getValue/setValue, and the
 *     resampling branch (:52-69) through StructuredVolumeView + serial::for_each with the
 *     destination-to-source coordinate mapping of :55-69.  Those few lines are the only
 *     reference logic restated here; sampling, clamping and the codec are the reference's.
 *
 * Volumes are allocated with 8 zeroed bytes behind the last voxel: the reference's
 * sampleLinear leaves hi.x unclamped (StructuredVolumeView.hpp:93-99) and reads one voxel
 * past the end for some destination voxels.  The padding keeps that read inside owned
 * memory; what it returns is still not a property of the reference, and the tests exclude
 * those voxels where the result can depend on it.
 */
#include <cstdint>
#include <cstring>

#include <vkt/Aggregates.hpp>
#include <vkt/Arithmetic.hpp>
#include <vkt/Copy.hpp>
#include <vkt/Histogram.hpp>
#include <vkt/Resample.hpp>
#include <vkt/StructuredVolume.hpp>
#include <vkt/Transform.hpp>
#include <vkt/Voxel.hpp>

#include "StructuredVolumeView.hpp"
#include "for_each.hpp"

#include "vkt_oracle.h"

namespace
{
    constexpr std::size_t kPad = 8;

    struct RefVolume : vkt::StructuredVolume
    {
        explicit RefVolume(const vko_volume* v)
            : vkt::StructuredVolume(v->dims[0], v->dims[1], v->dims[2], (vkt::DataFormat)v->fmt, 1.f, 1.f, 1.f,
                                    v->lo, v->hi)
            , bytes(getSizeInBytes())
        {
            resize(bytes + kPad); // ManagedBuffer::resize (protected)
            std::memcpy(getData(), v->data, bytes);
            std::memset(getData() + bytes, 0, kPad);
        }

        void store(vko_volume* v) { std::memcpy(v->data, getData(), bytes); }

        std::size_t bytes;
    };

    vkt::Vec3i vec(const int32_t a[3]) { return { a[0], a[1], a[2] }; }

    typedef vkt::Error (*ArithRange)(vkt::StructuredVolume&, vkt::StructuredVolume&, vkt::StructuredVolume&,
                                     vkt::Vec3i, vkt::Vec3i, vkt::Vec3i);
    const ArithRange kArith[10] = {
        vkt::SumRange,     vkt::DiffRange,     vkt::ProdRange,     vkt::QuotRange,     vkt::AbsDiffRange,
        vkt::SafeSumRange, vkt::SafeDiffRange, vkt::SafeProdRange, vkt::SafeQuotRange, vkt::SafeAbsDiffRange,
    };

    // TransformRange takes a plain function pointer: the caller's C callback is parked here
    // (unary form only: the reference declares the binary C++ TransformRange but defines none)
    thread_local vko_unary_op g_unary = nullptr;

    void unaryTrampoline(int32_t x, int32_t y, int32_t z, vkt::VoxelView v)
    {
        g_unary(x, y, z, v.bytes, (int32_t)v.dataFormat, v.mappingLo, v.mappingHi);
    }
} // namespace

extern "C" {

int32_t vkr_map(uint8_t* dst, float value, int32_t fmt, float lo, float hi)
{
    return (int32_t)vkt::MapVoxel(dst, value, (vkt::DataFormat)fmt, lo, hi);
}

int32_t vkr_unmap(float* value, const uint8_t* src, int32_t fmt, float lo, float hi)
{
    return (int32_t)vkt::UnmapVoxel(*value, src, (vkt::DataFormat)fmt, lo, hi);
}

/* n voxels at a stride of `bpv` bytes; dst bytes / values the reference leaves alone keep
 * what the caller put there */
void vkr_map_n(uint8_t* dst, const float* values, size_t n, size_t bpv, int32_t fmt, float lo, float hi)
{
    for (size_t i = 0; i < n; ++i)
        vkt::MapVoxel(dst + i * bpv, values[i], (vkt::DataFormat)fmt, lo, hi);
}

void vkr_unmap_n(float* values, const uint8_t* src, size_t n, size_t bpv, int32_t fmt, float lo, float hi)
{
    for (size_t i = 0; i < n; ++i)
        vkt::UnmapVoxel(values[i], src + i * bpv, (vkt::DataFormat)fmt, lo, hi);
}

void vkr_fill_range(vko_volume* v, const int32_t first[3], const int32_t last[3], float value)
{
    RefVolume vol(v);
    vkt::StructuredVolumeView view(vol);
    vkt::serial::for_each(first[0], last[0], first[1], last[1], first[2], last[2],
                          [=](int x, int y, int z) mutable { view.setValue(x, y, z, value); });
    vol.store(v);
}

int32_t vkr_copy_range(vko_volume* dst, vko_volume* src, const int32_t first[3], const int32_t last[3],
                       const int32_t dst_offset[3])
{
    RefVolume d(dst), s(src);
    vkt::Error err = vkt::CopyRange(d, s, vec(first), vec(last), vec(dst_offset));
    d.store(dst);
    return (int32_t)err;
}

int32_t vkr_arith_range(int32_t op, vko_volume* dst, vko_volume* s1, vko_volume* s2, const int32_t first[3],
                        const int32_t last[3], const int32_t dst_offset[3])
{
    if (op < 0 || op >= 10)
        return -1;
    RefVolume d(dst), a(s1), b(s2);
    vkt::Error err = kArith[op](d, a, b, vec(first), vec(last), vec(dst_offset));
    d.store(dst);
    return (int32_t)err;
}

void vkr_resample(vko_volume* dst, vko_volume* src, int32_t filter)
{
    RefVolume d(dst), s(src);
    vkt::FilterMode fm = filter == 1 ? vkt::FilterMode::Linear : vkt::FilterMode::Nearest;
    if (d.getDims() == s.getDims()) {
        // Resample_serial.hpp:32-48: no spatial resampling, per-voxel re-encode
        vkt::Vec3i dims = d.getDims();
        for (int32_t z = 0; z != dims.z; ++z)
            for (int32_t y = 0; y != dims.y; ++y)
                for (int32_t x = 0; x != dims.x; ++x)
                    d.setValue(x, y, z, s.getValue(x, y, z));
    } else {
        // Resample_serial.hpp:52-69: the float coordinates convert to sampleLinear's int32_t
        // parameters implicitly, as they do there
        vkt::StructuredVolumeView dstView(d);
        vkt::StructuredVolumeView srcView(s);
        const vkt::Vec3i dd = d.getDims(), sd = s.getDims();
        const bool linear = fm == vkt::FilterMode::Linear;
        vkt::serial::for_each(0, dd.x, 0, dd.y, 0, dd.z, [=](int x, int y, int z) mutable {
            // f32 divide by the destination extent, then f32 multiply by the source extent
            const float fx = x / float(dd.x) * sd.x;
            const float fy = y / float(dd.y) * sd.y;
            const float fz = z / float(dd.z) * sd.z;
            const float value = linear ? srcView.sampleLinear(fx, fy, fz)
                                       : srcView.getValue((int32_t)fx, (int32_t)fy, (int32_t)fz);
            dstView.setValue(x, y, z, value);
        });
    }
    d.store(dst);
}

int32_t vkr_aggregates_range(const vko_volume* v, const int32_t first[3], const int32_t last[3],
                             vko_aggregates* out)
{
    RefVolume vol(v);
    vkt::Aggregates a;
    vkt::Error err = vkt::ComputeAggregatesRange(vol, a, vec(first), vec(last));
    out->min = a.min;
    out->max = a.max;
    out->mean = a.mean;
    out->stddev = a.stddev;
    out->var = a.var;
    out->sum = a.sum;
    out->prod = a.prod;
    out->argmin[0] = a.argmin.x;
    out->argmin[1] = a.argmin.y;
    out->argmin[2] = a.argmin.z;
    out->argmax[0] = a.argmax.x;
    out->argmax[1] = a.argmax.y;
    out->argmax[2] = a.argmax.z;
    return (int32_t)err;
}

/* The reference indexes its bin array unchecked: the caller must only pass voxels whose bin
 * lies in [0, num_bins). */
int32_t vkr_histogram_range(const vko_volume* v, const int32_t first[3], const int32_t last[3], uint64_t* bins,
                            uint64_t num_bins)
{
    RefVolume vol(v);
    vkt::Histogram h(num_bins);
    vkt::Error err = vkt::ComputeHistogramRange(vol, h, vec(first), vec(last));
    const std::size_t* counts = h.getBinCounts();
    for (uint64_t i = 0; i < num_bins; ++i)
        bins[i] = counts[i];
    return (int32_t)err;
}

int32_t vkr_transform_range1(vko_volume* v, const int32_t first[3], const int32_t last[3], vko_unary_op op)
{
    RefVolume vol(v);
    g_unary = op;
    vkt::Error err = vkt::TransformRange(vol, first[0], first[1], first[2], last[0], last[1], last[2], unaryTrampoline);
    vol.store(v);
    return (int32_t)err;
}

} // extern "C"
