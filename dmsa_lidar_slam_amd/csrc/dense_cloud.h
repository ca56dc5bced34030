// dense_cloud.h — launchers of the kernels behind include/dmsa_dense_cloud.h (csrc/dense_cloud.hip): per-point pose interpolation and
// placement, the cross-scan voxel set, the stable compaction and the 12- or 16-byte rows of the binary PCD.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dmsa {

// the trajectory in HBM: stamps[n_p], pos[n_p][3], quat[n_p][4] as (w, x, y, z) unit quaternions -- the order d_slerp_quat reads
struct DenseTraj {
    const double* stamps;
    const double* pos;
    const double* quat;
    int32_t n_p;
};
// the gates of rules 1-6 (include/dmsa_dense_cloud.h)
struct DenseGates {
    float l2i[12];  // rows 0..2 of lidar_to_imu, row-major: (c0, c1, c2, c3) per row
    float min_range, max_range;
    double time_offset, max_pose_gap;
    float voxel_size;
};
// per-call counters in HBM, zeroed before every scan
enum DenseCounter { DC_NON_FINITE = 0, DC_OUT_OF_RANGE, DC_OUT_OF_TIME, DC_IN_GAP, DC_OUT_OF_GRID, DC_THINNED, DC_PROBE_FAILED, DC_COUNT };

struct VoxelSlot {
    unsigned long long key;    // three biased 21-bit cells; ~0 = empty (a key has 63 bits)
    unsigned long long owner;  // scan_no << 32 | point index of the first point that fell in the voxel; ~0 = none yet
};
constexpr int kDensePoseLds = 5;       // poses (= 4 segments) a workgroup of k_dense_place keeps in LDS
constexpr int kVoxelProbeBound = 256;  // slots a probe visits before it gives up (the table is never more than half full)

// rules 3-4 for n stamps: pose12 (n x 12, may be null), segment (n, may be null)
void launch_dense_interpolate(DenseTraj tr, double max_pose_gap, const double* t, int64_t n, double* pose12, int32_t* segment, hipStream_t s);
// rules 1-6 up to the key: g[i] = placed point (w = 1), keep[i] = 1 iff the point passed, key[i] = its voxel key (voxel_size > 0);
// keep[n] = 0 (the scan over n + 1 flags ends in the total).  origin (may be null): origin[i] = rule 5 for the sensor-frame point (0, 0, 0) with
// point i's pose (w = 1), the sensor origin of include/dmsa_dense_normals.h.  intensity: g[i].w = xyz[i].w, bit for bit, instead of 1
// (include/dmsa_dense_intensity.h, I3) -- an instantiation of its own, the other one is the kernel as it was
void launch_dense_place(const float4* xyz, const double* stamps, int64_t n, DenseTraj tr, DenseGates g, float4* placed, int32_t* keep,
                        unsigned long long* key, unsigned long long* counters, float4* origin, bool intensity, hipStream_t s);
// pass A: find or claim the slot of every kept point, atomicMin of (scan_no, i) on its owner word; slot_of[i] = the slot, -1 = none
void launch_voxel_claim(const int32_t* keep, const unsigned long long* key, int64_t n, uint32_t scan_no, VoxelSlot* table, uint64_t mask, int32_t* slot_of,
                        unsigned long long* counters, hipStream_t s);
// pass B: keep[i] &= owner of its slot == (scan_no, i)
void launch_voxel_resolve(int32_t* keep, const int32_t* slot_of, int64_t n, uint32_t scan_no, const VoxelSlot* table, unsigned long long* counters,
                          hipStream_t s);
// takes the scan out of the table again: the slots its survivors own were empty before it
void launch_voxel_rollback(const int32_t* keep, const int32_t* slot_of, int64_t n, VoxelSlot* table, hipStream_t s);
void launch_voxel_clear(VoxelSlot* table, uint64_t slots, hipStream_t s);
// every occupied slot of `from` into `to` (empty, larger); a probe that runs out counts in counters[DC_PROBE_FAILED]
void launch_voxel_rehash(const VoxelSlot* from, uint64_t from_slots, VoxelSlot* to, uint64_t to_mask, unsigned long long* counters, hipStream_t s);
// stable compaction: out[scan_excl[i]] = placed[i] for keep[i] != 0
void launch_dense_scatter(const float4* placed, const int32_t* keep, const int32_t* scan_excl, int64_t n, float4* out, hipStream_t s);
// row_floats = 3: rows[3 k .. 3 k + 2] = out[k].xyz; 4: rows[4 k .. 4 k + 3] = out[k] (x y z intensity).  label != nullptr: rows of one more
// word, the bits of label[k] behind the floats (include/dmsa_dense_clusters.h, C7)
void launch_dense_pack_rows(const float4* out, const int32_t* label, int64_t m, int row_floats, float* rows, hipStream_t s);

}  // namespace dmsa
