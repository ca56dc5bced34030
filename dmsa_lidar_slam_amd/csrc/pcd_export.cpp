// pcd_export.cpp — include/dmsa_wire_formats.h, the map side: PointCloud.pcd rows formatted by csrc/pcd_kernels.hip, chunk by chunk.
// (The header text is host work: dmsa_pcd_header_pointnormal in wire_formats.cpp; the way of a chunk from the device to the file: copy_back.h.)
#include "copy_back.h"

// scratch of the PCD export; allocated on first use, bounded by the chunk, independent of the resident problem
struct PcdState {
    DevBuf in_xyz, in_normal, in_curv, dec, len, off, scan_tmp;
    CopyBack text;      // the text of a chunk, worst case of its rows
    PinnedBuf h_total;  // int32, one byte count per slot
};

void pcd_release(dmsa_ctx* ctx) {
    delete ctx->pcd;  // (its buffers and events release themselves)
    ctx->pcd = nullptr;
}

namespace {

constexpr int64_t kDefaultChunkRows = (int64_t)1 << 18;  // 26.25 MiB of text at most per buffer

struct PcdSource {
    const float* xyz;        // host n x 4, or null: the resident global points
    const float* normal;     // host n x 4, or null: the resident global normals (keyframe model)
    const float* curvature;  // host n, or null: 0
    int64_t first;           // first row of whatever is resident
};

int pcd_state(dmsa_ctx* ctx, PcdState** out) {
    if (!ctx->pcd) {
        PcdState* st = new (std::nothrow) PcdState();
        if (!st) return DMSA_ERR_NOMEM;
        ctx->pcd = st;
        HIPCHK(st->h_total.ensure(2 * sizeof(int32_t), nullptr));
        HIPCHK(st->text.create());
    }
    *out = ctx->pcd;
    return DMSA_OK;
}

// every argument check of the two entry points, BEFORE anything is launched
int pcd_check(dmsa_ctx* ctx, const PcdSource& src, int64_t n) {
    if (!ctx || n < 0 || src.first < 0) return DMSA_ERR_INVALID;
    if (!src.xyz && ctx->model == MODEL_NONE) return fail(ctx, DMSA_ERR_INVALID, "pcd: xyz == NULL needs a resident problem");
    if (!src.normal && ctx->model != MODEL_KEYFRAMES)
        return fail(ctx, DMSA_ERR_INVALID, "pcd: normal == NULL needs a resident keyframe problem (the window model has no normals)");
    if ((!src.xyz || !src.normal) && (src.first > ctx->n || n > ctx->n - src.first)) return fail(ctx, DMSA_ERR_INVALID, "pcd: rows beyond the resident problem");
    return DMSA_OK;
}

// chunk rows [at, at + n) of the call -> device pointers of their inputs (staged into the scratch where they are not resident and contiguous)
int pcd_stage(dmsa_ctx* ctx, PcdState* st, const PcdSource& src, int64_t at, int64_t n, const float4** xyz, const float4** normal, const float** curv) {
    const size_t bytes = (size_t)n * 16;
    const int64_t r0 = src.first + at;
    if (src.xyz) {
        HIPCHK(st->in_xyz.ensure(bytes));
        HIPCHK(hipMemcpyAsync(st->in_xyz.p, src.xyz + 4 * at, bytes, hipMemcpyHostToDevice, ctx->stream));
        *xyz = st->in_xyz.as<float4>();
    } else if (ctx->model == MODEL_WINDOW && r0 + n > ctx->N) {
        // static points are not moved by updateGlobalPoints: they sit in the local array (dmsa_get_global_points)
        HIPCHK(st->in_xyz.ensure(bytes));
        const int64_t moving = std::max<int64_t>(0, ctx->N - r0);
        if (moving > 0) HIPCHK(hipMemcpyAsync(st->in_xyz.p, ctx->d_global.as<float4>() + r0, (size_t)moving * 16, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(st->in_xyz.as<float4>() + moving, ctx->d_local.as<float4>() + r0 + moving, (size_t)(n - moving) * 16, hipMemcpyDeviceToDevice, ctx->stream));
        *xyz = st->in_xyz.as<float4>();
    } else {
        *xyz = ctx->d_global.as<float4>() + r0;
    }
    if (src.normal) {
        HIPCHK(st->in_normal.ensure(bytes));
        HIPCHK(hipMemcpyAsync(st->in_normal.p, src.normal + 4 * at, bytes, hipMemcpyHostToDevice, ctx->stream));
        *normal = st->in_normal.as<float4>();
    } else {
        *normal = ctx->d_nglobal.as<float4>() + r0;
    }
    *curv = nullptr;
    if (src.curvature) {
        HIPCHK(st->in_curv.ensure((size_t)n * 4));
        HIPCHK(hipMemcpyAsync(st->in_curv.p, src.curvature + at, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        *curv = st->in_curv.as<float>();
    }
    return DMSA_OK;
}

// enqueue on the library stream: decode + row offsets of chunk rows [at, at + n); the chunk's byte count goes to h_total[slot]
int pcd_enqueue_offsets(dmsa_ctx* ctx, PcdState* st, const PcdSource& src, int64_t at, int64_t n, int slot) {
    const float4 *xyz, *normal;
    const float* curv;
    CHK(pcd_stage(ctx, st, src, at, n, &xyz, &normal, &curv));
    HIPCHK(st->dec.ensure((size_t)n * kPcdValues * 8));
    HIPCHK(st->len.ensure((size_t)(n + 1) * 4));
    HIPCHK(st->off.ensure((size_t)(n + 1) * 4));
    HIPCHK(st->scan_tmp.ensure(scan_temp_bytes((size_t)n + 1)));
    launch_pcd_decode(xyz, normal, curv, n, st->dec.as<uint64_t>(), st->len.as<int32_t>(), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(exclusive_scan_i32(st->scan_tmp.p, st->scan_tmp.cap, st->len.as<int32_t>(), st->off.as<int32_t>(), (size_t)n + 1, ctx->stream));
    HIPCHK(hipMemcpyAsync(st->h_total.as<int32_t>() + slot, st->off.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    return DMSA_OK;
}
// ... and the text of the chunk just decoded into text.dev[slot] (which holds the worst case of n rows)
int pcd_enqueue_render(dmsa_ctx* ctx, PcdState* st, int64_t n, int slot) {
    HIPCHK(st->text.dev[slot].ensure((size_t)n * kPcdMaxRowBytes + 16));
    launch_pcd_render(st->dec.as<uint64_t>(), st->off.as<int32_t>(), n, st->text.dev[slot].as<char>(), ctx->stream);
    HIPCHK(hipGetLastError());
    return DMSA_OK;
}

int64_t chunk_rows_of(int64_t requested) { return requested <= 0 ? kDefaultChunkRows : std::min(requested, kPcdMaxChunkRows); }

int save_pcd(dmsa_ctx* ctx, PcdFile& file, const PcdSource& src, int64_t n, int64_t chunk) {
    PcdState* st = nullptr;
    CHK(pcd_state(ctx, &st));
    char header[512];
    const int hn = dmsa_pcd_header_pointnormal(n, header, (int32_t)sizeof(header));
    if (hn < 0) return hn;
    if (!file.write(header, (size_t)hn)) return fail(ctx, DMSA_ERR_INVALID, file.why());
    auto rows_of = [&](int64_t c) { return std::min(chunk, n - c * chunk); };
    for (int b = 0; b < 2; ++b) HIPCHK(st->text.reserve(b, 0, (size_t)std::min(chunk, n) * kPcdMaxRowBytes));  // (the device side: pcd_enqueue_render)
    auto format = [&](int64_t c, int b) -> int {
        CHK(pcd_enqueue_offsets(ctx, st, src, c * chunk, rows_of(c), b));
        return pcd_enqueue_render(ctx, st, rows_of(c), b);
    };
    auto bytes_of = [&](int64_t, int b, size_t* bytes) -> int {  // known once the chunk's offsets are: the host reads them
        HIPCHK(st->text.wait_produced(b));
        return *bytes = (size_t)st->h_total.as<int32_t>()[b], DMSA_OK;
    };
    return copy_back_chunks(ctx, st->text, file, (n + chunk - 1) / chunk, format, bytes_of);
}

}  // namespace

extern "C" {

int dmsa_format_pcd_rows(dmsa_ctx* ctx, const float* xyz, const float* normal, const float* curvature, int64_t first, int64_t n, char* out, int64_t cap,
                         int64_t* bytes_out) {
    if (bytes_out) *bytes_out = 0;
    const PcdSource src{xyz, normal, curvature, first};
    CHK(pcd_check(ctx, src, n));
    if (!bytes_out || cap < 0 || (cap > 0 && !out)) return DMSA_ERR_INVALID;
    if (n == 0) return DMSA_OK;
    CHK(set_device(ctx));
    PcdState* st = nullptr;
    CHK(pcd_state(ctx, &st));
    // one chunk after the other; once the text no longer fits, only the byte counts of the remaining chunks are computed
    int64_t bytes = 0;
    bool fits = true;
    for (int64_t at = 0; at < n; at += kDefaultChunkRows) {
        const int64_t rows = std::min(kDefaultChunkRows, n - at);
        CHK(pcd_enqueue_offsets(ctx, st, src, at, rows, 0));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        const int64_t total = st->h_total.as<int32_t>()[0];
        fits = fits && bytes + total <= cap;
        if (fits && total > 0) {
            CHK(pcd_enqueue_render(ctx, st, rows, 0));
            HIPCHK(hipMemcpyAsync(out + bytes, st->text.dev[0].p, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
        bytes += total;
    }
    *bytes_out = bytes;
    return fits ? DMSA_OK : fail(ctx, DMSA_ERR_INVALID, "pcd: capacity too small (bytes_out holds the bytes needed)");
}

int dmsa_save_pcd_ascii_ex(dmsa_ctx* ctx, const char* path, const float* xyz, const float* normal, const float* curvature, int64_t n, int64_t chunk_rows,
                           int64_t* bytes_written) {
    if (bytes_written) *bytes_written = 0;
    const PcdSource src{xyz, normal, curvature, 0};
    CHK(pcd_check(ctx, src, n));
    if (!path || !bytes_written) return DMSA_ERR_INVALID;
    if (n == 0) return fail(ctx, DMSA_ERR_INVALID, "pcd: an empty cloud is not written (pcl::PCDWriter::writeASCII refuses it)");
    CHK(set_device(ctx));
    PcdFile file;
    if (!file.open(path, "pcd")) return fail(ctx, DMSA_ERR_INVALID, file.why());
    const int rc = copy_back_end(ctx, file, save_pcd(ctx, file, src, n, chunk_rows_of(chunk_rows)));
    *bytes_written = file.bytes();  // (what a failed call wrote stays)
    return rc;
}

int dmsa_save_pcd_ascii(dmsa_ctx* ctx, const char* path, const float* xyz, const float* normal, const float* curvature, int64_t n, int64_t* bytes_written) {
    return dmsa_save_pcd_ascii_ex(ctx, path, xyz, normal, curvature, n, 0, bytes_written);
}

}  // extern "C"
