// copy_back.h — how rows made on the device reach a file, for all three writers (pcd_export.cpp, dense_store.cpp, dense_cloud_api.cpp):
// two slots, each a device buffer, a pinned buffer and two events.  A producer on the library stream fills a slot's device buffer, the side
// stream copies it into the slot's pinned buffer, the host writes the other slot's pinned buffer meanwhile.
// THE REUSE RULE: a slot's device buffer is produced into again only after wait_copied() of its last copy, its pinned buffer copied into again
// only after the host is done with it (its fwrite).  Slots taken in turn, each written before the next but one is produced, keep it.
// Internal.  The owner makes its device current before create() and before the object dies (as for PinnedBuf).
#pragma once
#include "dmsa_ctx.h"
#include "pcd_file.h"

class CopyBack {
public:
    DevBuf dev[2];  // what the producer writes into
    ~CopyBack() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() {  // once, before the first use
        for (hipEvent_t& e : ev)
            if (hipError_t rc = e ? hipSuccess : hipEventCreateWithFlags(&e, hipEventDisableTiming); rc != hipSuccess) return rc;
        return hipSuccess;
    }
    // slot b holds dev_bytes on the device and host_bytes pinned (a pinned block that has to grow is allocated with host_alloc: the caller's slack)
    hipError_t reserve(int b, size_t dev_bytes, size_t host_bytes, size_t host_alloc = 0) {
        if (hipError_t rc = dev[b].ensure(dev_bytes); rc != hipSuccess) return rc;
        return host[b].ensure(host_bytes, nullptr, host_alloc);  // (null: by the rule every earlier copy was waited for)
    }
    // behind everything `from` holds now: slot b is produced ...
    hipError_t produced(int b, hipStream_t from) { return hipEventRecord(ev[b], from); }
    hipError_t wait_produced(int b) { return hipEventSynchronize(ev[b]); }  // ... and the host has seen it (a producer that tells the host the byte count)
    // the first `bytes` of slot b to its pinned buffer, on `side`, behind "produced"
    hipError_t copy_back(int b, size_t bytes, hipStream_t side) {
        if (bytes > dev[b].cap || bytes > host[b].cap) return hipErrorInvalidValue;
        if (hipError_t rc = hipStreamWaitEvent(side, ev[b], 0); rc != hipSuccess) return rc;
        if (hipError_t rc = hipMemcpyAsync(host[b].p, dev[b].p, bytes, hipMemcpyDeviceToHost, side); rc != hipSuccess) return rc;
        return hipEventRecord(ev[2 + b], side);
    }
    hipError_t wait_copied(int b, const void** rows) { return *rows = host[b].p, hipEventSynchronize(ev[2 + b]); }  // the host may read *rows

private:
    PinnedBuf host[2];
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // produced[2], copied[2]
};

// `chunks` >= 1 chunks through `back` into `file`, chunk c in slot c & 1.  produce(c, slot) enqueues the kernels of chunk c on the library
// stream; bytes_of(c, slot, &bytes) gives its size once it is enqueued (it may wait_produced for it).  Round c:
//   stream2  copy-back(c)   |   host  waits for copy-back(c - 1)   |   device  produce(c + 1)   |   host  write(c - 1)
// so chunk c + 1 goes into the slot of chunk c - 1 after that chunk's copy was waited for, and is copied back after its write: the rule.
template <class Produce, class BytesOf>
int copy_back_chunks(dmsa_ctx* ctx, CopyBack& back, PcdFile& file, int64_t chunks, Produce produce, BytesOf bytes_of) {
    auto enqueue = [&](int64_t c) -> int {
        CHK(produce(c, (int)(c & 1)));
        HIPCHK(back.produced((int)(c & 1), ctx->stream));
        return DMSA_OK;
    };
    size_t bytes[2] = {0, 0};
    CHK(enqueue(0));
    for (int64_t c = 0; c <= chunks; ++c) {  // (round `chunks` writes the last chunk)
        const int b = (int)(c & 1);
        const void* rows = nullptr;
        if (c < chunks) {
            CHK(bytes_of(c, b, &bytes[b]));
            HIPCHK(back.copy_back(b, bytes[b], ctx->stream2));
        }
        if (c > 0) HIPCHK(back.wait_copied(b ^ 1, &rows));
        if (c + 1 < chunks) CHK(enqueue(c + 1));
        if (c > 0 && !file.write(rows, bytes[b ^ 1])) return fail(ctx, DMSA_ERR_INVALID, file.why());
    }
    return DMSA_OK;
}

// The end of a call that wrote all of `file`, `rc` its status so far: nothing of a failed call may still be in flight when the caller's arrays
// go away; a call that succeeded closes the file, which can fail too.  What a failed call leaves of the file is the caller's choice.
inline int copy_back_end(dmsa_ctx* ctx, PcdFile& file, int rc) {
    if (rc != DMSA_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->stream2);
    } else if (!file.close()) {
        rc = fail(ctx, DMSA_ERR_INVALID, file.why());
    }
    return rc;
}
