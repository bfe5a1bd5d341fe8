// Device and page-locked host memory for the callers of libiqdemod.so (include/iqdemod.h: iqd_dev_*, iqd_host_*), and the
// front end alone.
#include "iqd_engine_impl.h"

extern "C" {

int iqd_dev_alloc(iqd_t *e, size_t bytes, void **out)
{
    if (!e || !out) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    if (hipMalloc(out, bytes) != hipSuccess) return e->fail(IQD_ENOMEM, "hipMalloc(%zu) failed", bytes);
    return IQD_OK;
}

int iqd_dev_free(iqd_t *e, void *p)
{
    if (!e) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipFree(p));
    return IQD_OK;
}

int iqd_dev_upload(iqd_t *e, void *dst, const void *src, size_t bytes)
{
    if (!e) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

int iqd_dev_download(iqd_t *e, void *dst, const void *src, size_t bytes)
{
    if (!e) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

// The front end alone: what the reference leaves in the caller's buffer / sends from its IQ dump tap.
int iqd_front_end_device(iqd_t *e, uint32_t first_ch, uint32_t n_ch, const void *iq_dev, size_t bytes_per_ch,
                         void *out_dev)
{
    if (!range_ok(e, first_ch, n_ch) || !iq_dev || !out_dev) return e ? e->fail(IQD_EINVAL, "bad channel range or NULL buffer") : IQD_EINVAL;
    if (bytes_per_ch == 0 || bytes_per_ch % 8 != 0)   // the rotation pattern spans 4 samples (IqDataProcessor.cc:567-611)
        return e->fail(IQD_EINVAL, "bytes_per_ch (%zu) must be a positive multiple of 8", bytes_per_ch);
    if ((((uintptr_t)iq_dev) | ((uintptr_t)out_dev)) & 7) return e->fail(IQD_EINVAL, "buffers must be 8-byte aligned");
    (void)hipSetDevice(e->device);
    {
        std::lock_guard<std::mutex> lk(e->mu);
        int rc = upload_params(e);
        if (rc != IQD_OK) return rc;
    }
    HIP_TRY(e, launch_front_end((const uint8_t *)iq_dev, (int8_t *)out_dev, e->d_params, first_ch, n_ch, bytes_per_ch, e->stream));
    return IQD_OK;
}

int iqd_front_end(iqd_t *e, uint32_t first_ch, uint32_t n_ch, const uint8_t *iq, size_t bytes_per_ch, int8_t *out)
{
    if (!range_ok(e, first_ch, n_ch) || !iq || !out) return e ? e->fail(IQD_EINVAL, "bad channel range or NULL buffer") : IQD_EINVAL;
    (void)hipSetDevice(e->device);
    const size_t bytes = (size_t)n_ch * bytes_per_ch;
    HIP_TRY(e, e->st_iq.ensure(bytes));
    HIP_TRY(e, e->st_pcm.ensure(bytes));
    HIP_TRY(e, hipMemcpyAsync(e->st_iq.p, iq, bytes, hipMemcpyHostToDevice, e->stream));
    int rc = iqd_front_end_device(e, first_ch, n_ch, e->st_iq.p, bytes_per_ch, e->st_pcm.p);
    if (rc != IQD_OK) return rc;
    HIP_TRY(e, hipMemcpyAsync(out, e->st_pcm.p, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

int iqd_host_alloc(iqd_t *e, size_t bytes, void **out)
{
    if (!e || !out || bytes == 0) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        *out = nullptr;
        return e->fail(IQD_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
    }
    return IQD_OK;
}

int iqd_host_free(iqd_t *e, void *p)
{
    if (!e) return IQD_EINVAL;
    if (p) (void)hipHostFree(p);
    return IQD_OK;
}

int iqd_dev_tile(iqd_t *e, void *dst, size_t period, size_t total)
{
    if (!e || !dst || period == 0 || period % 16 || total % 16 || total < period) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    HIP_TRY(e, launch_tile_fill((uint8_t *)dst, period, total, e->stream));
    return IQD_OK;
}

// IqDataProcessor::upconvertByFsOver4 / downconvertByFsOver4 (IqDataProcessor.cc:487-611) as the reference offers
// them: in place, on signed bytes, a multiple of 8 of them.
int iqd_convert_fs_over_4(iqd_t *e, int direction, int8_t *buffer, size_t byte_count)
{
    if (!e || !buffer) return e ? e->fail(IQD_EINVAL, "NULL buffer") : IQD_EINVAL;
    if (direction != 1 && direction != -1) return e->fail(IQD_EINVAL, "direction must be +1 (up) or -1 (down)");
    if (byte_count == 0 || byte_count % 8 != 0) return e->fail(IQD_EINVAL, "byte_count (%zu) must be a positive multiple of 8", byte_count);
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    HIP_TRY(e, e->st_iq.ensure(byte_count));
    HIP_TRY(e, hipMemcpyAsync(e->st_iq.p, buffer, byte_count, hipMemcpyHostToDevice, s));
    HIP_TRY(e, launch_rotate_signed(e->st_iq.as<int8_t>(), byte_count, direction, s));
    HIP_TRY(e, hipMemcpyAsync(buffer, e->st_iq.p, byte_count, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return IQD_OK;
}

}  // extern "C"
