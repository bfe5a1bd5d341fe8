/* include/iqdemod.h — C-ABI of libiqdemod.so, the MI355X-native IQ demodulation engine.
 *
 * This is the drop-in boundary for the RtlSdrDiags per-sample DSP hot path.  Each entry
 * point names the reference interface it replaces (paths relative to the reference's
 * radioDiags/ directory).  Signatures are plain C: pointers, sizes and scalars only.
 *
 * One engine owns N independent channels.  Each channel behaves like one reference
 * IqDataProcessor with its four demodulators attached (hdr_diags/IqDataProcessor.h:16-93):
 * it keeps its own mode, gains, squelch threshold/tracker and per-demodulator filter state.
 * A channel's input is the same offset-binary uint8 interleaved I/Q the reference receives
 * (256 kS/s) and its output the same 8 kS/s S16 PCM (bytes/64 samples per accepted block).
 *
 * Threading (IqDataProcessor.h:35-37, DataConsumer.cc:342): one thread at a time may be
 * inside iqd_accept_*() for a given engine; setters may be called from another thread
 * between or during accepts and take effect at the next accept (they are mutex-guarded).
 *
 * All functions returning int return IQD_OK (0) or a negative IQD_E* code.
 */
#ifndef IQDEMOD_H
#define IQDEMOD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IQD_ABI_VERSION 1

/* IqDataProcessor::demodulatorType, hdr_diags/IqDataProcessor.h:20 */
enum iqd_mode {
    IQD_MODE_NONE = 0, IQD_MODE_AM = 1, IQD_MODE_FM = 2,
    IQD_MODE_WBFM = 3, IQD_MODE_LSB = 4, IQD_MODE_USB = 5
};

/* Which demodulator a gain applies to: {Am,Fm,WbFm,Ssb}Demodulator::setDemodulatorGain */
enum iqd_demod { IQD_DEMOD_AM = 1, IQD_DEMOD_FM = 2, IQD_DEMOD_WBFM = 3, IQD_DEMOD_SSB = 4 };

enum iqd_status {
    IQD_OK = 0,
    IQD_EINVAL = -1,      /* bad argument (range, alignment, NULL) */
    IQD_ENODEV = -2,      /* no usable HIP device / HIP runtime error at create */
    IQD_ENOMEM = -3,      /* host or device allocation failed */
    IQD_EHIP = -4,        /* a HIP call failed during accept (see iqd_last_error) */
    IQD_ESTATE = -5,      /* exact-state verification could not be repaired (never expected) */
    IQD_EALREADY = -6     /* iqd_agc_enable: every channel of the range already was in that state */
};

typedef struct iqd_engine iqd_t;

typedef struct iqd_config {
    uint32_t abi_version;   /* IQD_ABI_VERSION */
    uint32_t n_channels;    /* >= 1 */
    uint32_t block_bytes;   /* squelch / acceptIqData granularity per channel.  0 -> 32768
                               (Radio.cc:16, 1895).  Multiple of 256, <= 32768 (the cap of
                               SignalDetector.h:49).  A call SHORTER than this is one short block
                               (a short USB read, Radio.cc:1895-1906): any multiple of 64 bytes - 32
                               samples, one PCM sample, the period of the chains' /32 commutators
                               (the reference itself strides 8 bytes, IqDataProcessor.cc:567-611) -
                               in every mode. */
    int32_t device;         /* HIP device ordinal, -1 -> current device */
    uint32_t flags;         /* IQD_F_* */
    uint32_t reserved[3];
} iqd_config;

#define IQD_F_NO_MAGNITUDE 0x1u /* do not produce per-block magnitudes when no channel's squelch can close
                                   (the reference only reports them through an optional callback) */
/* Every chain (WBFM, FM, AM, SSB) exists as two kernels with identical results: tiles (one workgroup per run of
 * samples) and a streaming pipeline (one persistent workgroup per CU, used for launches big enough to fill the chip,
 * squelch-gated ones included).  These two flags pin the choice for all chains (tests, A/B measurements; the names
 * are from the round in which only WBFM had both); the environment variable IQD_WBFM_PATH=tiles|stream does the same.
 * A call with several families whose streaming pipelines all apply runs them as ranges of ONE launch's workgroups
 * (stats.mixed_launches), each family on a share of the CUs chosen so that all of them end together (per-family segment
 * lengths and lead-ins taken into account; IQD_SHARES=cost: in plain proportion to the estimated cost, the earlier rule).
 * More environment variables exist for measurements only, read once by iqd_create: IQD_MIXED=forked runs such a call's
 * families as kernels of their own on side streams instead (the round-2 arrangement), IQD_FULL_GRID=1 then gives every
 * family all CUs in turn instead of a share of them side by side, IQD_FAMILY_WEIGHTS=am,fm,wbfm,ssb replaces the
 * relative cost estimates, IQD_STREAM_WGS=<n> fixes the streaming kernels' workgroup count, IQD_STREAM_GRAN / IQD_D4_GRAN=128|256|512
 * the granule of the WBFM / the other pipelines' segment lengths (defaults 512 / 128), IQD_STREAM_MIN_SEG=<samples> replaces the
 * measured per-family thresholds (samples a launch must bring per segment of the persistent workgroups before it streams),
 * IQD_AM_STREAM_MIN=<PCM samples> the shortest AM / SSB row that may stream (128), IQD_FAMILY_NS=am,fm,wbfm,ssb the ns per
 * segment sample the share planner works with. */
#define IQD_F_WBFM_TILES  0x2u
#define IQD_F_WBFM_STREAM 0x4u
/* Squelch-gated iqd_accept_iq_device calls (some channel's threshold can reject a block) read their input twice: a pre-pass
 * takes every block's magnitude and makes the decisions (Squelch.cc:227-273), then the pipelines walk the open blocks.  With
 * this flag the pre-pass of a call runs on a stream of the engine's own, ordered only behind the PREVIOUS call's pre-pass, so
 * that it overlaps the previous call's pipelines (a continuous stream of calls: magnitudes one call ahead).  The caller
 * promises in return that `iq_dev` is complete when the call is MADE - ordering its producer on iqd_stream() is not enough,
 * the pre-pass does not wait there - and that it does not reuse the small output buffers (pcm_count / magnitude /
 * signal_present) of the call before.  Host-pointer calls ignore the flag.  Results are identical. */
#define IQD_F_PREPASS_OVERLAP 0x8u

/* Replaces: new IqDataProcessor(...) + new {Am,Fm,WbFm,Ssb}Demodulator(pcmCallback) +
 * set*Demodulator() wiring, Radio.cc:150-181.  Every channel starts like the reference:
 * mode None (IqDataProcessor.cc:38), squelch threshold -200 dBFS (:41), receive gain 24 dB
 * (Radio.cc:325-328), default demodulator gains, zero filter state. */
int iqd_create(const iqd_config *cfg, iqd_t **out);
void iqd_destroy(iqd_t *e);

/* Replaces IqDataProcessor::setDemodulatorMode, IqDataProcessor.cc:236-262
 * (Lsb/Usb also select the SsbDemodulator sideband, :244-256). */
int iqd_set_mode(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int mode);

/* Replaces {Am,Fm,WbFm,Ssb}Demodulator::setDemodulatorGain (e.g. WbFmDemodulator.cc:341-348).  Takes effect with the
 * first sample of the next accept; what the filters already hold keeps the gain it was made with, exactly as in the
 * reference, for ANY sequence of changes: the engine keeps every change whose samples can still reach a filter
 * history (up to 64 per channel and demodulator - a change needs an accept of >= 32 samples in between, and the
 * histories reach back 2048 samples). */
int iqd_set_gain(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int demod, float gain);

/* Replaces IqDataProcessor::setSignalDetectThreshold, IqDataProcessor.cc:284-295. */
int iqd_set_squelch(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int32_t threshold_dbfs);

/* Replaces the global radio_adjustableReceiveGainInDb read at IqDataProcessor.cc:765
 * (per channel here, because each channel stands for its own receiver). */
int iqd_set_rx_gain_db(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t gain_db);

/* Reads the IF gain in force for a channel (it differs from the last value set once the channel's AGC has run). */
int iqd_get_rx_gain_db(iqd_t *e, uint32_t ch, uint32_t *gain_db);

/* Replaces AutomaticGainControl (hdr_diags/AutomaticGainControl.h:22-47, src_diags/AutomaticGainControl.cc), one
 * per channel, constructed as Radio.cc:184 does (operating point -12 dBFS, Harris type, alpha 0.8, deadband 1,
 * blanking limit 1, disabled).  An enabled AGC receives the channel's block magnitudes in block order - the
 * reference's signalMagnitudeCallback, IqDataProcessor.cc:781-790 -> AutomaticGainControl.cc:47-64 - and moves
 * the channel's IF gain (Radio::setReceiveIfGainInDb, Radio.cc:817-868), which the squelch of the NEXT block
 * compares with (IqDataProcessor.cc:765).  The recorded samples themselves do not change with the gain: there
 * is no tuner behind a channel here - except a channelizer channel that follows its gain ("Gain-following channels"
 * below: the channelizer applies the IF gain per block).  Each setter mirrors the reference method of the same name and returns
 * IQD_EINVAL where that method returns false (setType :287-320, setDeadband :351-369, setBlankingLimit :399-420,
 * setOperatingPoint :440-448, setAgcFilterCoefficient :475-493, enable/disable :516-595). */
enum iqd_agc_type { IQD_AGC_LOWPASS = 0, IQD_AGC_HARRIS = 1 };
int iqd_agc_set_type(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t type);
int iqd_agc_set_deadband(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t deadband_db);     /* 0..10 */
int iqd_agc_set_blanking_limit(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t limit);      /* 0..10 */
int iqd_agc_set_operating_point(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int32_t dbfs);
int iqd_agc_set_filter_coefficient(iqd_t *e, uint32_t first_ch, uint32_t n_ch, float coefficient); /* [0.001, 0.999) */
int iqd_agc_enable(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int enabled);   /* IQD_EALREADY where enable()/disable() return false */

/* displayInternalInformation() (AutomaticGainControl.cc:1082-1149) as values. */
typedef struct iqd_agc_state {
    uint32_t enabled, type;
    int32_t operating_point_dbfs;
    uint32_t deadband_db, blanking_limit;
    float alpha;
    uint32_t rx_gain_db;            /* the receiver's IF gain in force */
    uint32_t if_gain_db;            /* the AGC's own copy (ifGainInDb) */
    float filtered_if_gain_db;
    uint32_t blanking_counter, gain_was_adjusted;
    int32_t normalized_level_dbfs;
    uint32_t signal_magnitude;      /* last magnitude the AGC acted on */
} iqd_agc_state;
int iqd_agc_get_state(iqd_t *e, uint32_t ch, iqd_agc_state *out);

/* Replaces FrequencyScanner (hdr_diags/FrequencyScanner.h:33-75, src_diags/FrequencyScanner.cc), one per channel,
 * idle at 162.55 MHz like the reference's constructor (:96-131).  A scanning channel advances its frequency by the
 * increment on every block its squelch rejects - the reference's signalStateCallback -> run(), :47-62, :378-404 -
 * and wraps from the end to the start frequency; every such step is one Radio::setReceiveFrequency command, which
 * the host forwards to its tuner (nothing retunes recorded bytes).  iqd_scanner_set_parameters mirrors
 * setScanParameters (:190-218, refused while scanning), iqd_scanner_start(…, 1/0) mirrors start()/stop()
 * (:240-310; the first start after new parameters jumps to the END frequency); both return IQD_EALREADY where the
 * reference returns false for every channel of the range. */
int iqd_scanner_set_parameters(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint64_t start_hz, uint64_t end_hz,
                               uint64_t increment_hz);
int iqd_scanner_start(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int start);
/* The frequency the channel's radio was last told to tune to, the number of tuning commands so far, isScanning(). */
int iqd_scanner_get(iqd_t *e, uint32_t ch, uint64_t *current_hz, uint64_t *tune_count, int *scanning);

/* Optional record of the IF gain each block's squelch compared with, for the channels and blocks of the last
 * accept call: [n_ch][n_blocks], host memory. */
int iqd_set_gain_trace(iqd_t *e, int enabled);
int iqd_get_gain_trace(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t *gain_db, size_t n_blocks);
/* With the same switch: the frequency each channel was tuned to after each block, [n_ch][n_blocks]. */
int iqd_get_frequency_trace(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint64_t *hz, size_t n_blocks);

/* Front-end rotation selector: +1 = upconvertByFsOver4 (what acceptIqData applies,
 * IqDataProcessor.cc:749, the default), -1 = downconvertByFsOver4 (:496-540), 0 = none. */
int iqd_set_rotation(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int rotation);
/* (The reference has no such switch.  A selector changed in mid-stream takes effect with the first sample of the next
 * accept; what the filters already hold keeps the old rotation, as in-place rotation at acceptance time would.) */

/* Replaces {Am,Fm,WbFm,Ssb}Demodulator::resetDemodulator() for all four demodulators of the
 * channels (note WbFmDemodulator.cc:304-320 leaves the de-emphasis filter state alone). */
int iqd_reset(iqd_t *e, uint32_t first_ch, uint32_t n_ch);
/* The same for one demodulator only (demod = IQD_DEMOD_*), as the reference's per-object call. */
int iqd_reset_demod(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int demod);

/* Replaces IqDataProcessor::acceptIqData(timeStamp, bufferPtr, byteCount),
 * IqDataProcessor.cc:722-840, for n_ch channels at once, each receiving
 * bytes_per_ch / block_bytes consecutive calls' worth of data.
 *
 *   iq             [n_ch][bytes_per_ch] uint8, channel-major; NOT modified (the reference
 *                  mutates its buffer in place; callers that relied on that must not).
 *   bytes_per_ch   multiple of block_bytes, or one short block (see iqd_config::block_bytes).
 *   pcm            [n_ch][bytes_per_ch/64] int16; channel c's samples are packed at the front
 *                  of its row (squelched blocks contribute nothing, like the reference's
 *                  callback, IqDataProcessor.cc:793).
 *   pcm_count      [n_ch] number of valid PCM samples per channel (may be NULL).
 *   magnitude      [n_ch][bytes_per_ch/block_bytes] SignalDetector::signalMagnitude per block
 *                  = what registerSignalMagnitudeCallback would deliver (may be NULL).
 *   signal_present [n_ch][bytes_per_ch/block_bytes] Squelch::run() result per block = what
 *                  registerSignalStateCallback would deliver (may be NULL).
 *
 * Host-pointer form: copies in, runs, copies out, returns when done (large calls are sliced and
 * double-buffered so that the copies overlap the kernels; the result is the same). */
int iqd_accept_iq(iqd_t *e, uint32_t first_ch, uint32_t n_ch,
                  const uint8_t *iq, size_t bytes_per_ch,
                  int16_t *pcm, uint32_t *pcm_count,
                  uint32_t *magnitude, uint8_t *signal_present);

/* Device-pointer form: every pointer is HIP device memory (same layouts); the work is
 * enqueued on the engine's stream and the call returns as soon as it is queued (the WBFM
 * hand-off verification and, if ever needed, its repair run on the device).  Keep the
 * buffers alive and use iqd_synchronize() - or synchronise iqd_stream() - before reading
 * results.  Until then the PCM rows are the call's own: the AM / SSB pipelines keep intermediate
 * (detector) values there before the DC-removal pass turns them into PCM in place. */
int iqd_accept_iq_device(iqd_t *e, uint32_t first_ch, uint32_t n_ch,
                         const void *iq_dev, size_t bytes_per_ch,
                         void *pcm_dev, void *pcm_count_dev,
                         void *magnitude_dev, void *signal_present_dev);

int iqd_synchronize(iqd_t *e);

/* Replaces {Am,Fm,WbFm,Ssb}Demodulator::acceptIqData(int8_t *bufferPtr, uint32_t bufferLength) - AmDemodulator.h:30,
 * FmDemodulator.h:30, WbFmDemodulator.h:31 (WbFmDemodulator.cc:383-411), SsbDemodulator.h:33 - the demodulator's own
 * entry, which the processor calls behind its squelch (IqDataProcessor.cc:793-836) and the reference's offline harness
 * calls directly (demodulatorResearch/demodulators/demod.cc:262-285):
 *   iq            [n_ch][bytes_per_ch] SIGNED interleaved I/Q as the processor hands it over (after the -128 and the
 *                 rotation); NOT modified (the reference's WBFM chain filters its buffer in place)
 *   bytes_per_ch  any positive multiple of 64 (32 samples = one PCM sample); the reference's own limit of 32768 per call
 *                 (demodulatedData[16384]) does not apply
 *   pcm           [n_ch][bytes_per_ch/64]: every sample reaches the demodulator - no squelch, no signal or magnitude
 *                 notification, no AGC or scanner step; the channel's squelch tracker does not move
 * The demodulators are the ones the channel's processor uses (Radio.cc:150-181): their filter state is shared with
 * iqd_accept_iq of the same channel, in either order.  demod = IQD_DEMOD_*; the SSB sideband is the one last selected
 * by iqd_set_mode(LSB / USB) or iqd_demod_set_sideband - SsbDemodulator::setLsbDemodulationMode / setUsbDemodulationMode
 * (SsbDemodulator.cc:333-367; the reference's constructor starts in LSB, :143). */
int iqd_demod_accept(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int demod,
                     const int8_t *iq, size_t bytes_per_ch, int16_t *pcm);
int iqd_demod_set_sideband(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int lsb);

/* The front end alone, IqDataProcessor.cc:735-749: s = u - 128, then the channel's rotation; [n_ch][bytes_per_ch]
 * signed bytes out.  This is what the reference leaves in the caller's buffer (it works in place) and what its
 * IQ dump tap streams (:756-760, UdpClient::sendData); iqd_accept_* itself never modifies its input. */
int iqd_front_end(iqd_t *e, uint32_t first_ch, uint32_t n_ch, const uint8_t *iq, size_t bytes_per_ch, int8_t *out);
int iqd_front_end_device(iqd_t *e, uint32_t first_ch, uint32_t n_ch, const void *iq_dev, size_t bytes_per_ch,
                         void *out_dev);
/* Replaces IqDataProcessor::upconvertByFsOver4 (direction +1, IqDataProcessor.cc:567-611) and
 * downconvertByFsOver4 (direction -1, :487-531; hdr_diags/IqDataProcessor.h:32-33) as stand-alone calls: `buffer`
 * holds SIGNED interleaved I/Q, is rotated in place (-(-128) stays -128), byte_count a multiple of 8. */
int iqd_convert_fs_over_4(iqd_t *e, int direction, int8_t *buffer, size_t byte_count);

/* Diagnostics (the reference's displayInternalInformation() text dumps, e.g.
 * IqDataProcessor.cc:860-926, become queryable values). */
typedef struct iqd_stats {
    uint64_t accepts;            /* iqd_accept_* calls */
    uint64_t samples;            /* IQ samples accepted, all channels */
    uint64_t kernel_launches;    /* chain-kernel launches */
    uint64_t state_checks;       /* tile hand-offs verified bit-exact (WBFM de-emphasis) */
    uint64_t state_repairs;      /* tiles (WBFM) / rows (AM, SSB DC removal) re-run from the exact carried state */
    double chain_kernel_ms;      /* HIP-event time of the chain kernels while profiling is on */
    uint64_t chain_kernel_count; /* launches covered by chain_kernel_ms */
    uint64_t segment_repairs;    /* extra in-kernel passes of the segmented de-emphasis (a segment's warm-up had not
                                    reached its neighbour's exact state yet) */
    uint64_t stream_launches;    /* chain launches (any family) that ran as a streaming pipeline */
    uint64_t device_launches;    /* kernel-launch calls queued by iqd_accept_* (all kinds) */
    uint64_t device_copies;      /* memcpy / memset operations queued by iqd_accept_* */
    uint64_t mixed_launches;     /* calls whose families' streaming pipelines ran as ranges of one launch */
} iqd_stats;

int iqd_get_stats(iqd_t *e, iqd_stats *out);
int iqd_set_profiling(iqd_t *e, int enabled);  /* HIP events around the chain kernels */
int iqd_get_channel_mode(iqd_t *e, uint32_t ch, int *mode);
int iqd_get_channel_gain(iqd_t *e, uint32_t ch, int demod, float *gain);
const char *iqd_last_error(iqd_t *e);
const char *iqd_strerror(int status);
uint32_t iqd_abi_version(void);

/* The reference's stand-alone resampler classes (not used by any demodulator), block-wise and for
 * n_channels independent streams at once.  A resampler replaces, per channel, one object of
 *   IQD_RESAMPLE_DECIMATE_F32     Decimator(filterLength, coefficients, decimationFactor), Filters/Decimator.cc:
 *                                 one output per `factor` inputs, when the last of them arrives (:283-321);
 *   IQD_RESAMPLE_INTERPOLATE_F32  Interpolator(...), Filters/Interpolator.cc: `factor` outputs per input (:340-364);
 *   IQD_RESAMPLE_INTERPOLATE_I16  Interpolator_int16(...), Filters/Int16/Interpolator_int16.cc: the same in Q15
 *                                 with the per-MAC clamp (:203-246); int16 in and out,
 * and a call with n_in samples per channel replaces n_in decimate()/interpolate() calls; the filter state (and the
 * decimator's commutator phase) carries over to the next call.  Layouts: in [n_channels][n_in], out
 * [n_channels][iqd_resampler_out_count(r, n_in)].  iqd_resampler_reset = resetFilterState(). */
enum iqd_resample_kind { IQD_RESAMPLE_DECIMATE_F32 = 0, IQD_RESAMPLE_INTERPOLATE_F32 = 1, IQD_RESAMPLE_INTERPOLATE_I16 = 2 };
typedef struct iqd_resampler iqd_resampler_t;
int iqd_resampler_create(iqd_t *e, int kind, const float *taps, uint32_t n_taps, uint32_t factor, uint32_t n_channels,
                         iqd_resampler_t **out);
void iqd_resampler_destroy(iqd_resampler_t *r);
int iqd_resampler_reset(iqd_resampler_t *r);
size_t iqd_resampler_out_count(const iqd_resampler_t *r, size_t n_in);
int iqd_resampler_run(iqd_resampler_t *r, const void *in, size_t n_in, void *out);                 /* host pointers */
int iqd_resampler_run_device(iqd_resampler_t *r, const void *in_dev, size_t n_in, void *out_dev);  /* queued on the engine's stream */

/* The reference's four hot-path filter classes (layer L0) stand-alone, block-wise and for n_channels
 * independent streams at once, with the caller's own coefficients.  A filter replaces, per channel, one object of
 *   IQD_FILTER_DECIMATE_I16  Decimator_int16(filterLength, coefficients, decimationFactor), Filters/Int16/Decimator_int16.cc
 *                            :176-238, :310-351: n counts samples since create / reset, an output when n = factor - 1
 *                            (mod factor): acc = 1 << 14; for k = 0 .. L-1 in this order acc += hq[k] x[n-k], clamped to
 *                            [-2^30, 2^30 - 1] after EVERY MAC; y = (int16)(acc >> 15).  1 <= factor <= 64, 1 <= L <= 1024;
 *   IQD_FILTER_FIR_I16       FirFilter_int16(...), Filters/Int16/FirFilter_int16.cc:151-213: the same with an output for
 *                            every input (factor must be 1);
 *   IQD_FILTER_FIR_F32       FirFilter(...), Filters/FirFilter.cc:144-185: y = 0, then y = y + h[k] x[n-k] for k ascending,
 *                            every product and sum rounded to float.  1 <= L <= 1024, factor 1;
 *   IQD_FILTER_IIR_F32       IirFilter(...), Filters/IirFilter.cc:161-229: v = the FIR_F32 sum over num; r = 0, then
 *                            r = r + den[k] y[n-1-k] for k ascending; y[n] = v - r.  den excludes the leading 1 (the DC
 *                            blocker is num {1, -1}, den {-0.95}).  1 <= n_num <= 64, 1 <= n_den <= 64, factor 1,
 * and a call with n_in samples per channel replaces n_in decimate() / filterData() calls.  x[n < 0] = 0.  The state carries
 * over from call to call per channel: the FIR history, the decimator's commutator phase, the IIR's past inputs and
 * outputs; iqd_filter_reset = resetFilterState().  The I16 kinds quantise num like the reference's constructors (round(32768
 * h) cast to int16: a tap of 1.0 becomes -32768).  den / n_den are NULL / 0 for the three FIR kinds.
 *
 * Layouts: in [n_channels][n_in], out [n_channels][iqd_filter_out_count(f, n_in)]; int16 elements for the I16 kinds, float
 * for the F32 kinds.  0 <= n_in <= 2^31 - 1; a decimator call may yield no output.  Device pointers need only the element's
 * alignment (the kernels stage 16 bytes per lane where every row happens to be 16-byte aligned, with identical results).
 * Results are bit for bit the reference's for finite inputs (for NaN / Inf the bit pattern is unspecified); float
 * subnormals are kept, not flushed.
 *
 * Refusals, each IQD_EINVAL with a message naming the argument, before anything is allocated or queued: a NULL pointer, kind
 * out of range, n_num / n_den / factor outside the ranges above (factor != 1 where it must be 1, den given to a FIR kind or
 * missing for IIR_F32), n_channels = 0, n_in above 2^31 - 1.
 *
 * IIR_F32 is serial in time and exact (no scan, no warm-up overlap: both would change the rounding for arbitrary
 * coefficients): one lane per channel, one wave per 64 channels.  Fewer than 64 x (number of CUs) channels therefore cannot
 * fill the device.
 *
 * Host only, no GPU:
 *   iqd_filter_tile_samples     the input samples (IIR: time steps) one workgroup stages per tile for these sizes, 0 for
 *                               sizes out of range - where calls of T - 1, T and T + 1 samples take different paths;
 *   iqd_filter_clamp_free_taps  the largest K0 <= n_taps with sum over k < K0 of |hq[k]| <= 32767: up to tap K0 no partial
 *                               sum can leave [-2^30, 2^30 - 1] for any int16 input (2^14 + 32768 x 32767 < 2^30), so the
 *                               kernel sums that prefix with packed dot products and clamps only from K0 on. */
enum iqd_filter_kind { IQD_FILTER_DECIMATE_I16 = 0, IQD_FILTER_FIR_I16 = 1, IQD_FILTER_FIR_F32 = 2, IQD_FILTER_IIR_F32 = 3 };
typedef struct iqd_filter iqd_filter_t;
int iqd_filter_create(iqd_t *e, int kind, const float *num, uint32_t n_num, const float *den, uint32_t n_den, uint32_t factor,
                      uint32_t n_channels, iqd_filter_t **out);
void iqd_filter_destroy(iqd_filter_t *f);
int iqd_filter_reset(iqd_filter_t *f);
size_t iqd_filter_out_count(const iqd_filter_t *f, size_t n_in);
int iqd_filter_run(iqd_filter_t *f, const void *in, size_t n_in, void *out);                 /* host pointers */
int iqd_filter_run_device(iqd_filter_t *f, const void *in_dev, size_t n_in, void *out_dev);  /* queued on the engine's stream */
uint32_t iqd_filter_tile_samples(int kind, uint32_t n_num, uint32_t n_den, uint32_t factor);
uint32_t iqd_filter_clamp_free_taps(const float *taps, uint32_t n_taps);

/* Wideband channelizer: many engine channels cut out of one capture (uint8 here; int8 and int16: "Signed captures" below) at M x 256 kS/s (an RTL-SDR at 2.048 MS/s is
 * M = 8).  The reference gets its one channel from the RTL2832U's own down-converter (Radio tunes the dongle, the chip
 * delivers 256 kS/s around that frequency); this is the same front for any number of channels of one receiver.  Every
 * step after the phasor table is integer and fixed here, so results are exact, not within a tolerance:
 *
 *   sources   a call gives each of n_sources sources bytes_per_source bytes of interleaved offset-binary I/Q, layout
 *             [n_sources][bytes_per_source]; x[n] = (I - 128) + j (Q - 128); n counts samples since create / reset;
 *             x[n < 0] = 0 (zero history, like Decimator_int16).  bytes_per_source: a multiple of 64 M.
 *   prototype h[0..K) int16 Q15 low-pass, 1 <= K <= 1024, |h[k]| <= 32639, 256 sum |h| <= 2^31 - 256 (else IQD_EINVAL).
 *             taps == NULL: iqd_channelizer_default_taps(M).
 *   phasor    P[i] = (lrint(32767 cos(2 pi i / 4096)), lrint(32767 sin(2 pi i / 4096))), i < 4096:
 *             iqd_channelizer_phasor_table.
 *   channel c source s_c, phase increment d_c (uint32), gain shift L_c in [0, 8].  Offset f_c = int32(d_c) / 2^32 Fs_wide.
 *             Complex taps: i_k = (k d_c mod 2^32) >> 20, gr[k] = (h[k] Pc[i_k] + 2^14) >> 15,
 *             gi[k] = (h[k] Ps[i_k] + 2^14) >> 15 (>> is an arithmetic shift throughout).
 *   output m  n = m M + M - 1 (the decimator's emit point, Decimator_int16.cc:310-351), m counts since create / reset:
 *             Ar = sum_k gr[k] xr[n-k] - gi[k] xi[n-k],  Ai = sum_k gr[k] xi[n-k] + gi[k] xr[n-k]   (exact in int32)
 *             a = sat16((A + 128) >> 8) on each rail
 *             (c, s) = P[(n d_c mod 2^32) >> 20]                   (e^{-j w n}: the channel to DC; no phase state)
 *             rr = ar c + ai s,  ri = ai c - ar s,  y = sat8((r + 2^(21-L)) >> (22-L)),  byte = y + 128
 *             L = 0 is unity gain (full-scale DC in, full scale out); every step of L adds 6 dB.
 *   out       [n_channels][bytes_per_source / M] uint8: exactly the rows iqd_accept_iq_device reads.
 *
 * The reference tunes the dongle to station + Fs/4 (Radio.cc:617-618), and the engine's default rotation (+1) brings
 * that back.  So a channel placed at station + 64 kHz feeds the default rotation exactly as the dongle would; a channel
 * placed on the station itself wants iqd_set_rotation(..., 0).
 *
 * iqd_channelizer_set_channels takes effect at the next run and rebuilds only the named channels' taps (every channel
 * starts on source 0, increment 0, L = 0).  Runs are queued on the engine's stream; run_device returns once queued, the
 * host forms return when done.  iqd_accept_wideband: uploads only the wideband bytes, channelizes into rows the
 * channelizer owns, runs iqd_accept_iq_device for engine channels [first_ch, first_ch + n_channels) and copies the
 * results out (layouts of iqd_accept_iq; the rows, bytes_per_source / M, follow its block_bytes rule).
 * Every out-of-range argument is IQD_EINVAL before anything is queued. */
typedef struct iqd_channelizer_config {
    uint32_t n_sources;     /* >= 1 */
    uint32_t n_channels;    /* >= 1 */
    uint32_t decimation;    /* M, 2..64; with decimation_den > 1: P */
    uint32_t n_taps;        /* K, 1..1024 (1..1024 Q); ignored when taps == NULL */
    const int16_t *taps;    /* h[0..K), Q15; NULL -> iqd_channelizer_default_taps(M) */
    uint32_t decimation_den; /* Q: 0 or 1 (integer decimation), 2, 4, 8 (fractional, below) */
    uint32_t sample_format; /* IQD_WIDE_U8 (0, the above), IQD_WIDE_S8, IQD_WIDE_S16 ("Signed captures" below) */
    uint32_t reserved[2];   /* 0 */
} iqd_channelizer_config;
typedef struct iqd_channelizer iqd_channelizer_t;
int iqd_channelizer_create(iqd_t *e, const iqd_channelizer_config *cfg, iqd_channelizer_t **out);
void iqd_channelizer_destroy(iqd_channelizer_t *z);   /* before its engine's iqd_destroy */
int iqd_channelizer_reset(iqd_channelizer_t *z);
int iqd_channelizer_set_channels(iqd_channelizer_t *z, uint32_t first, uint32_t n, const uint32_t *source,
                                 const uint32_t *phase_inc, const uint8_t *gain_shift);
/* wide_dev [n_sources][bytes_per_source] and out_dev [n_channels][bytes_per_source / M]: device memory, both 16-byte
 * aligned (else IQD_EINVAL) - the kernel reads and writes whole 16-byte units. */
int iqd_channelizer_run_device(iqd_channelizer_t *z, const void *wide_dev, size_t bytes_per_source, void *out_dev);
int iqd_channelizer_run(iqd_channelizer_t *z, const uint8_t *wide, size_t bytes_per_source, uint8_t *out);
int iqd_accept_wideband(iqd_t *e, iqd_channelizer_t *z, uint32_t first_ch, const uint8_t *wide, size_t bytes_per_source,
                        int16_t *pcm, uint32_t *pcm_count, uint32_t *magnitude, uint8_t *signal_present);
/* Host only, no GPU needed: the phasor table as (cos, sin) pairs, and the library's default prototype for M (odd length,
 * symmetric, DC gain 32768, passband +-100 kHz at the output rate, >= 50 dB down from 156 kHz: a Kaiser-windowed sinc
 * of 13 M + 1 taps).  default_taps returns the tap count (writing min(count, capacity) taps), or IQD_EINVAL. */
int iqd_channelizer_phasor_table(int16_t out[8192]);
int iqd_channelizer_default_taps(uint32_t decimation, int16_t *out, uint32_t capacity);

/* Fractional decimation: captures at P / Q x 256 kS/s, Q = decimation_den in {2, 4, 8}, gcd(P, Q) = 1, 2 <= P / Q <= 64
 * (2.4 MS/s is 75/8, 1.92 MS/s 15/2, 2.88 MS/s 45/4, 3.2 MS/s 25/2; else IQD_EINVAL).  Fs_wide = 256000 P / Q, which is
 * what a channel's offset f_c = int32(d_c) / 2^32 Fs_wide refers to.  decimation_den = 0 or 1 is the integer channelizer
 * above, bit for bit.  Everything not named here is as above:
 *
 *   prototype h[0..K) is given at the rate Q Fs_wide = 256000 P.  Branch r (0 <= r < Q) is h_r[k] = h[k Q + r],
 *             k < ceil((K - r) / Q); a branch may be empty.  1 <= K, ceil(K / Q) <= 1024, |h[k]| <= 32639 and, for every
 *             branch, 256 sum_k |h_r[k]| <= 2^31 - 256.  taps == NULL: iqd_channelizer_default_taps_q(P, Q).
 *   output m  u = m P + P - 1, n = floor(u / Q) (the newest wide sample it uses), r = u mod Q; m counts since create /
 *             reset.  Complex taps of the branch on its own sample delays: i_k = (k d_c mod 2^32) >> 20,
 *             gr_r[k] = (h_r[k] Pc[i_k] + 2^14) >> 15, gi_r likewise; A = sum_k g_r[k] x[n - k]; then a, the rotation by
 *             P[(n d_c mod 2^32) >> 20], y and the byte exactly as above.  An output of an empty branch is 0x80 0x80.
 *   length    bytes_per_source: a multiple of 64 P (32 P wide samples, 32 Q outputs), so every call starts on u mod Q =
 *             P - 1.  out and the rows of iqd_accept_wideband* are [n_channels][bytes_per_source Q / P]; the engine's
 *             block_bytes rule applies to that row length.
 *   default   iqd_channelizer_default_taps_q(P, Q): the design of iqd_channelizer_default_taps with M replaced by P
 *             (13 P + 1 taps, cut-off 124 kHz at the rate 256000 P), quantised per branch: q_r = lrint(w_r / sum(w_r)
 *             32768) and the first largest tap of each branch takes 32768 - sum(q_r), so that every branch has DC gain
 *             exactly 32768: unity gain at L = 0 and no gain ripple at the output rate.  Q = 0 or 1:
 *             iqd_channelizer_default_taps(P) tap for tap.  Host only, no GPU.
 *   scanner   channels of a fractional channelizer cannot follow a scanner: iqd_channelizer_follow_scanner(z, ..., 1)
 *             returns IQD_EINVAL.  iqd_channelizer_tuning is for integer M only. */
int iqd_channelizer_default_taps_q(uint32_t decimation, uint32_t den, int16_t *out, uint32_t capacity);

/* Signed captures: iqd_channelizer_config.sample_format says what a source's bytes are.  IQD_WIDE_U8 (0) is the RTL-SDR's
 * offset binary, everything above bit for bit.  IQD_WIDE_S8 is signed int8 (HackRF), IQD_WIDE_S16 little-endian signed
 * int16 (SDRplay, Airspy, USRP, the baseband recordings of SDR++, SDR# and SDRangel); any other value is IQD_EINVAL.  B is
 * the bytes per rail, 1 or 2.  Everything not named here is the integer channelizer's spec above:
 *
 *   sources   a source's bytes are interleaved I, Q of the format (int16: little-endian); x[n] = I + j Q with the values
 *             as they are: S8 I, Q in [-128, 127] (the capture u8 ^ 0x80 is the same signal as u8), S16 in [-32768, 32767].
 *             x[n < 0] = 0.  wide / wide_dev point at these bytes whatever the parameter's C type; wide_dev is 16-byte
 *             aligned as before.
 *   output m  taps g[k], n = m M + M - 1 and A = sum_k g[k] x[n - k] as above, A exact in unbounded integers (the S16 sum
 *             passes int32).  Stage a by format:
 *               S8   a = sat16((A + 128) >> 8), as U8
 *               S16  a = sat16((A + 2^15) >> 16) on each rail
 *             then the rotation, y and the byte as above.  So an S16 capture x16 = 256 x8 gives exactly the bytes of the
 *             8-bit capture x8: (256 A + 2^15) >> 16 = (A + 128) >> 8.  The tap conditions are unchanged.
 *   length    bytes_per_source: a multiple of 64 M B (32 M samples, 32 outputs).  out and the rows of
 *             iqd_accept_wideband* are [n_channels][bytes_per_source / (M B)]; the engine's block_bytes rule applies to
 *             that row length.
 *   works     fixed channels at integer M: iqd_channelizer_run / _run_device, iqd_accept_wideband / _device,
 *             set_channels between calls (retuning, moving), reset.
 *   not yet   each IQD_EINVAL before anything is queued, the message naming the format: decimation_den > 1 together with
 *             sample_format != 0 (at create); iqd_channelizer_follow_scanner(z, ..., 1); iqd_channelizer_set_survey with
 *             n_points > 0.
 * iqd_channelizer_window_outputs (host only, no GPU): the most outputs of one channel the kernel stages per workgroup
 * window, t with 2 B' (t M + Kp) <= 32768 bytes of LDS - Kp = K rounded up to 32, B' the byte planes of a sample rail
 * (U8, S8: 1; S16: 2) - cut to a multiple of 64 and to 1024 at most; 0 for arguments out of range. */
enum { IQD_WIDE_U8 = 0, IQD_WIDE_S8 = 1, IQD_WIDE_S16 = 2 };
uint32_t iqd_channelizer_window_outputs(uint32_t decimation, uint32_t n_taps, uint32_t sample_format);

/* Scanner-driven channels: a channelizer channel c may FOLLOW THE SCANNER of the engine channel it feeds in
 * iqd_accept_wideband*(e, z, first_ch, ...), e_c = first_ch + c.  A following channel's row of one call is split into the
 * engine's blocks (block_bytes, or the one short block); block b is cut by exactly the spec above with the increment d_b:
 *
 *   f_b       e_c's scanner frequency (iqd_scanner_get's current_hz) when block b begins: for b = 0 after the call's
 *             pending settings are applied (a start() after new parameters has already jumped to the end frequency -
 *             in the reference that tuning command precedes any data); for b > 0 after block b-1's squelch / scanner
 *             step (the engine's frequency-trace entry of block b-1).  Scanning or not: a stopped scanner leaves the
 *             channel where the scan stopped, as it would leave the dongle.
 *   centre    f_b + 64000 r, r = e_c's rotation selector in force for the call (+1, the default: the reference's
 *             "tune to station + Fs/4", Radio.cc:617-618).
 *   offset    o = f_b + 64000 r - F_s exactly (no wrap-around), Fs = 256000 M, F_s = the source's centre
 *             (iqd_channelizer_set_source_frequency, default 0).
 *   in band   -Fs/2 <= o < Fs/2: d_b = floor((o 2^32 + Fs/2) / Fs) mod 2^32 (floor division), and everything else -
 *             taps from d_b, the rotation P[(n d_b mod 2^32) >> 20] with absolute n, the gain shift, the history - as
 *             above.
 *   out of band  every byte of block b's row is 0x80 (silence: the squelch sees magnitude 0, the scanner moves on).
 *
 * This is the ideal retune: block b is cut at the frequency the scanner held when it began (the reference's dongle has
 * blocks in flight on USB when it retunes; that latency is not modelled).  The AGC keeps its meaning (the IF gain the
 * squelch compares with); it does not scale the channelizer's output.  The result is byte for byte what a host loop of
 * one-block calls gives that retunes every channel from iqd_scanner_get + iqd_channelizer_tuning, writes 0x80 over the
 * rows out of band and feeds iqd_accept_iq.  The decisions stay on the device: no host synchronisation per block, and
 * the number of launches per call does not grow with the number of blocks.
 *
 * iqd_channelizer_follow_scanner(z, first, n, 1 / 0): while a channel follows, its set_channels increment is kept but
 *             ignored (source and gain shift still apply); it is back in force at the next call after follow = 0.
 *             iqd_channelizer_run / run_device return IQD_EINVAL while any channel follows (no engine channel to follow);
 *             iqd_channelizer_reset keeps the following flags and source centres, as it keeps set_channels' values.
 * iqd_channelizer_tuning: the rule above as a host-only function (no GPU): IQD_EINVAL when out of band.
 * iqd_accept_wideband_device: iqd_accept_wideband with device pointers, queued on the engine's stream like
 *             iqd_accept_iq_device.  rows_dev [n_channels][bytes_per_source / M] (16-byte aligned, as wide_dev) is the
 *             caller's and holds the cut rows afterwards. */
int iqd_channelizer_set_source_frequency(iqd_channelizer_t *z, uint32_t first_source, uint32_t n, const uint64_t *centre_hz);
int iqd_channelizer_follow_scanner(iqd_channelizer_t *z, uint32_t first, uint32_t n, int follow);
int iqd_channelizer_tuning(uint32_t decimation, uint64_t source_centre_hz, uint64_t station_hz, int rotation, uint32_t *inc);
int iqd_accept_wideband_device(iqd_t *e, iqd_channelizer_t *z, uint32_t first_ch, const void *wide_dev, size_t bytes_per_source,
                               void *rows_dev, void *pcm_dev, void *pcm_count_dev, void *magnitude_dev, void *signal_present_dev);

/* Gain-following channels: a channelizer channel c may FOLLOW THE IF GAIN of the engine channel it feeds in
 * iqd_accept_wideband*(e, z, first_ch, ...), e_c = first_ch + c.  The channelizer stands where the reference's tuner
 * stands, so this closes the AGC's loop: the samples get louder or quieter, the next block's magnitude answers.  A
 * following channel's row of one call is split into the engine's blocks (block_bytes, or the one short block), as for
 * scanner-driven channels; block b is cut by exactly the integer spec above - taps, emit point, A, stage a, rotation,
 * history, absolute n - except that the last step uses a gain in dB instead of the shift L:
 *
 *   G_b       e_c's IF gain in force when block b begins: for b = 0 after the call's pending settings are applied
 *             (iqd_set_rx_gain_db, AGC one-shots); for b > 0 after block b-1's AGC step.  Exactly the value the engine's
 *             gain trace records for block b, the gain block b's squelch compares with.  With the AGC disabled it is the
 *             operator's manual gain: iqd_set_rx_gain_db is then a gain in dB for the channel (default 24).
 *   g_b       min(G_b, IQD_GAIN_FOLLOW_MAX = 48).  The squelch still subtracts the unclamped G_b: with the samples
 *             scaled, dBFS - gain is the antenna-referred level, as in the reference (IqDataProcessor.cc:765).
 *   split     e = g_b div 6, j = g_b mod 6, m_j = lrint(4096 2^(j/6)) = IQD_GAIN_M0 .. IQD_GAIN_M5.
 *   output    with r = rr or ri of the spec above (|r| < 2^31): t = floor(r m_j / 2^14),
 *             y = sat8((t + 2^(19-e)) >> (20-e)), byte = y + 128.
 *   identity  g = 6 L gives, byte for byte, the channel with gain shift L: floor(r / 4) + 2^(19-e) =
 *             floor((r + 2^(21-e)) / 4).  "6 dB" is therefore a factor of exactly 2 (6.0206 dB): a step of 6 in g is
 *             0.02 dB more than 6 dB, and the steps within are within 0.006 dB of 1 dB (m_j is rounded to 1 in 4096).
 *   floor     there is no gain below 0 dB: a channel whose carrier is near full scale at g = 0 stays there.
 *
 * The AGC's meaning is unchanged: the accept behind the channelizer re-derives the same decisions from the rows and moves
 * the real state; the channelizer steps a shadow of agc_run per block on the device, with no host synchronisation per block
 * and one launch per call whatever the block count.
 *
 * iqd_channelizer_follow_gain(z, first, n, 1 / 0): while a channel follows, its set_channels gain shift is kept but ignored
 *             (source and increment still apply); it is back in force at the next call after follow = 0.
 *             iqd_channelizer_reset keeps the flags.  follow = 0 on channels that do not follow is accepted.
 * IQD_EINVAL, before anything is queued: follow = 1 on a channelizer with decimation_den > 1 or sample_format != 0; follow = 1
 *             on a channel that follows its scanner, and iqd_channelizer_follow_scanner(..., 1) on a channel that follows
 *             its gain; iqd_channelizer_run / run_device while any channel follows its gain (no engine channel to
 *             follow); iqd_channelizer_survey* while any channel follows its gain. */
#define IQD_GAIN_FOLLOW_MAX 48
#define IQD_GAIN_M0 4096
#define IQD_GAIN_M1 4598
#define IQD_GAIN_M2 5161
#define IQD_GAIN_M3 5793
#define IQD_GAIN_M4 6502
#define IQD_GAIN_M5 7298
int iqd_channelizer_follow_gain(iqd_channelizer_t *z, uint32_t first, uint32_t n, int follow);

/* Band survey: where in the capture are the signals?  Per block and per point of a grid, the magnitude the squelch would
 * see - without placing channels, writing rows or running an accept.
 *
 *   point p   a virtual channel measured on EVERY source: increment d_p, gain shift L_p in [0, 8] (gain_shift == NULL: 0).
 *             iqd_channelizer_set_survey(z, n_points, ...): 0 <= n_points <= 4096, 0 clears the survey.  The points are
 *             independent of set_channels, of the following flags and of each other; iqd_channelizer_reset keeps them.
 *   result    magnitude[n_sources][n_blocks][n_points] uint32, n_blocks = row_bytes / block_bytes, row_bytes =
 *             bytes_per_source / M (bytes_per_source Q / P).  Entry (s, b, p) = floor(S / (block_bytes / 2)), S the sum
 *             over the block_bytes / 2 outputs of block b of SignalDetector's per-sample magnitude of the byte pair that a
 *             channel (source s, d_p, L_p) gets from the spec above (the fractional one for decimation_den > 1):
 *             a = |I - 128|, b = |Q - 128| (|-128| = 128), max(a, b) + (min(a, b) >> 1).  That is exactly the magnitude
 *             iqd_accept_wideband reports for such a channel with an engine whose block is block_bytes.
 *   state     a survey looks and does not touch: it reads the channelizer's current history and sample count and advances
 *             neither, so survey(x) followed by run(x) / accept_wideband(x) see the same samples.  Surveying bytes that
 *             were already run is the caller's error (they would be measured as if they followed themselves).
 *   lengths   bytes_per_source as for a run (a multiple of 64 M, of 64 P for fractional rates).  block_bytes, in row bytes:
 *             a multiple of 64 (decimation_den <= 1) or of 256 (decimation_den > 1), a divisor of row_bytes, at most 2^24.
 *             wide_dev and magnitude_dev: device memory, 16-byte aligned.
 *   refusals  IQD_EINVAL before anything is queued: any of the above violated, no points set, or any channel following
 *             its scanner.
 * The _device form is queued on the engine's stream and returns once queued; the host form returns when done.
 * iqd_magnitude_dbfs: host only, no GPU - the level the squelch compares (convertMagnitudeToDbFs: table entry of
 * min(magnitude, 127), minus 42), before any gain is subtracted, so that survey values can be held against thresholds. */
int iqd_channelizer_set_survey(iqd_channelizer_t *z, uint32_t n_points, const uint32_t *phase_inc, const uint8_t *gain_shift);
int iqd_channelizer_survey_device(iqd_channelizer_t *z, const void *wide_dev, size_t bytes_per_source, uint32_t block_bytes,
                                  void *magnitude_dev);
int iqd_channelizer_survey(iqd_channelizer_t *z, const uint8_t *wide, size_t bytes_per_source, uint32_t block_bytes,
                           uint32_t *magnitude);
int32_t iqd_magnitude_dbfs(uint32_t magnitude);

/* Band spectrum: an integer periodogram of the capture - every bin of the band at once, where the survey measures chosen
 * points through a whole channel filter.  A bin is a channelizer channel's stage A with M = K = N: the window times the
 * phasor table, summed over the frame's samples.  Every step is integer and fixed here, so results are exact:
 *
 *   sources   [n_sources][bytes_per_source], interleaved I/Q, one byte per rail.  IQD_WIDE_U8: x[n] = (I - 128) + j (Q - 128);
 *             IQD_WIDE_S8: the bytes as they are.  IQD_WIDE_S16 is refused (IQD_EINVAL, the message naming the format).
 *   frames    a frame is N consecutive samples; frames do not overlap.  No history, no state from call to call, no reset.
 *   N         n_bins: 64, 128, 256, 512, 1024 or 2048.
 *   window    w[0..N) int16, may be negative; |w[n]| <= 32639 and 256 sum |w| <= 2^31 - 256 (the channelizer's prototype
 *             conditions).  window == NULL: iqd_spectrum_default_window(N).
 *   phasor    P[i] = (Pc, Ps): iqd_channelizer_phasor_table, 4096 entries.
 *   bin k'    0 <= k' < N, q = k' - N / 2: rows run from low to high frequency, the centre frequency is bin N / 2.
 *             i(n) = ((q n) mod N) (4096 / N), the mod non-negative;
 *             c[n] = (w[n] Pc[i] + 2^14) >> 15,  s[n] = (w[n] Ps[i] + 2^14) >> 15   (>> arithmetic throughout)
 *             Ar = sum_n c[n] xr[n] + s[n] xi[n],  Ai = sum_n c[n] xi[n] - s[n] xr[n]      (exact in int32)
 *             ar = (Ar + 2^15) >> 16, ai likewise;  p = ar^2 + ai^2.  No saturation: |A| <= 128 x 1.4143 x 2^23 < 2^31, so
 *             |a| <= 23172 and p < 2^31.
 *   blocks    a block is F = frames_per_block consecutive frames, 1 <= F <= 2^24; bytes_per_source is a non-zero multiple
 *             of 2 N F; n_blocks = bytes_per_source / (2 N F).
 *   output    power[n_sources][n_blocks][N] uint32 = floor((sum over the block's frames of p) / F), the sum in 64 bits.
 *   default   iqd_spectrum_default_window(N): w[n] = (32767 - Pc[(2 n + 1) (2048 / N)]) >> sh, sh the smallest value >= 2
 *             with 256 sum w <= 2^31 - 256 - a Hann window with a half-sample offset, symmetric, integer only (sh = 2 up
 *             to N = 1024, 3 at N = 2048).
 *   full scale iqd_spectrum_full_scale(window, N): with c0[n] = (32767 w[n] + 2^14) >> 15,
 *             p_fs = ((127 sum_n c0[n] + 2^15) >> 16)^2: what bin N / 2 gives for the constant U8 input (255, 128).
 *             dBFS = 10 log10(max(p, 1) / p_fs).
 *   refusals  IQD_EINVAL with a message naming the argument, before anything is allocated or queued.  At create: a NULL
 *             pointer, n_sources = 0, n_bins outside the set, sample_format S16 or above 2, a non-zero reserved word, a
 *             window outside its bounds.  At run: frames_per_block 0 or above 2^24, bytes_per_source 0 or not a multiple
 *             of 2 N F, a NULL or misaligned device pointer, more (block, 64 bins) pairs than one launch covers (2^31 - 1).
 * A spectrum object is independent of channelizers: both may live on one engine and read the same device buffer.
 * wide_dev and power_dev: device memory, both 16-byte aligned.  The _device form is queued on the engine's stream and
 * returns once queued; the host form returns when done.  default_window and full_scale are host only, no GPU. */
typedef struct iqd_spectrum_config {
    uint32_t n_sources;     /* >= 1 */
    uint32_t n_bins;        /* N */
    const int16_t *window;  /* w[0..N); NULL -> iqd_spectrum_default_window(N) */
    uint32_t sample_format; /* IQD_WIDE_U8 or IQD_WIDE_S8 */
    uint32_t reserved[3];   /* 0 */
} iqd_spectrum_config;
typedef struct iqd_spectrum iqd_spectrum_t;
int iqd_spectrum_create(iqd_t *e, const iqd_spectrum_config *cfg, iqd_spectrum_t **out);
void iqd_spectrum_destroy(iqd_spectrum_t *s);   /* before its engine's iqd_destroy */
int iqd_spectrum_run_device(iqd_spectrum_t *s, const void *wide_dev, size_t bytes_per_source, uint32_t frames_per_block,
                            uint32_t *power_dev);
int iqd_spectrum_run(iqd_spectrum_t *s, const void *wide, size_t bytes_per_source, uint32_t frames_per_block, uint32_t *power);
int iqd_spectrum_default_window(uint32_t n_bins, int16_t *out);
int iqd_spectrum_full_scale(const int16_t *window, uint32_t n_bins, uint32_t *p_fs);   /* window NULL = the default */

/* Band activity: the occupied runs of a band spectrum - which stretches of the band stand above the noise floor, where each
 * is centred and how wide it is: the list iqd_channelizer_set_channels wants.  Every quantity is an unsigned integer and
 * every step is fixed here, so results are exact; there are no floats.
 *
 *   input     power[n_rows][N] uint32 in device memory: a row is what iqd_spectrum_run* wrote for one (source, block), but
 *             any values up to 2^32 - 1 are legal.  N = n_bins: 64, 128, 256, 512, 1024 or 2048.  Rows are independent: no
 *             state, no history, no reset.
 *   config    floor_rank r, 0 <= r < N;  ratio_q8 Q, 256 <= Q <= 2^24;  dc_guard d, 0 <= d <= N / 4;  bridge g, 0 <= g <= 64;
 *             min_width m, 1 <= m <= N;  max_detections K, 1 <= K <= N / 2;  reserved[0] = 0.
 *   floor     f = the r-th smallest of the row's N values, counted from 0, duplicates counted (r = N / 2: the upper
 *             median).  Guard bins are part of this count.
 *   threshold T = min(2^32 - 1, (max(f, 1) Q) >> 8), the product in 64 bits.
 *   hot       bin k is hot iff p[k] > T (strictly) and not (N / 2 - d < k < N / 2 + d): d = 0 guards nothing, d = 1 the centre
 *             bin only (an RTL-SDR's DC spike).
 *   runs      two hot bins i < j with no hot bin between them belong to one run iff j - i - 1 <= g; guard bins count as not
 *             hot; runs do not wrap from bin N - 1 to bin 0.  first / last: the run's lowest / highest hot bin,
 *             width = last - first + 1.  Runs of width < m are dropped and count nowhere.
 *   per run   over its hot bins only (a bridged gap or a guarded spike inside a run adds nothing): n_hot their number,
 *             peak_power the largest p, peak_bin the lowest bin that has it, sum_power = sum p (uint64),
 *             centroid_q8 = floor(256 sum k p[k] / sum p[k]), k the absolute bin.  sum p >= 1 (hot is p > T >= 0),
 *             sum k p < 2^54 and its 256-fold < 2^62: 64 bits hold them.
 *   output    rows[n_rows]: floor, threshold, n_found (every kept run, those past K too), n_hot_bins (every hot bin of
 *             the row, those of dropped runs too).  det[n_rows][K], ascending first_bin: the first min(n_found, K)
 *             records are the runs, the rest of the row's K records are all-zero bytes - both arrays are defined in full
 *             after a call.
 *   offset    iqd_detect_offset_hz(N, rate, centroid_q8): hz = floor(((centroid_q8 - 128 N) rate + 128 N) / (256 N)), floor
 *             also for negative numerators, in 64 bits: the offset from the capture's centre that iqd_channelizer_tuning
 *             takes (station = centre + hz).  Host only, no GPU.  IQD_EINVAL: hz NULL, N outside the set, rate 0,
 *             centroid_q8 >= 256 N.
 *   refusals  IQD_EINVAL with a message naming the argument, before anything is allocated or queued: a NULL pointer, a
 *             field outside its range, a non-zero reserved word; at run: n_rows 0 or above 2^31 - 1 (what one launch
 *             covers), a NULL or misaligned device pointer.
 * power_dev, rows_dev, det_dev: device memory, 16-byte aligned.  The _device form is queued on the engine's stream - straight
 * behind the iqd_spectrum_run_device that writes power_dev, with no synchronisation between them - and returns once queued;
 * the host form takes host pointers and returns when done. */
typedef struct iqd_detect_config {
    uint32_t n_bins;          /* N */
    uint32_t floor_rank;      /* r */
    uint32_t ratio_q8;        /* Q: the threshold over the floor, 256 = 1.0 */
    uint32_t dc_guard;        /* d */
    uint32_t bridge;          /* g */
    uint32_t min_width;       /* m */
    uint32_t max_detections;  /* K */
    uint32_t reserved[1];     /* 0 */
} iqd_detect_config;
typedef struct iqd_detect_row {
    uint32_t floor, threshold, n_found, n_hot_bins;
} iqd_detect_row;
typedef struct iqd_detection {
    uint32_t first_bin, last_bin, peak_bin, peak_power;
    uint64_t sum_power;
    uint32_t centroid_q8, n_hot;
} iqd_detection;
typedef struct iqd_detect iqd_detect_t;
int iqd_detect_create(iqd_t *e, const iqd_detect_config *cfg, iqd_detect_t **out);
void iqd_detect_destroy(iqd_detect_t *d);   /* before its engine's iqd_destroy */
int iqd_detect_run_device(iqd_detect_t *d, const uint32_t *power_dev, size_t n_rows, iqd_detect_row *rows_dev,
                          iqd_detection *det_dev);
int iqd_detect_run(iqd_detect_t *d, const uint32_t *power, size_t n_rows, iqd_detect_row *rows, iqd_detection *det);
int iqd_detect_offset_hz(uint32_t n_bins, uint32_t rate_hz, uint32_t centroid_q8, int64_t *hz);

/* Band tracks: the detector's runs followed from block to block - a stateful object behind iqd_detect_run_device on the same
 * stream.  For every (source, block) it writes S fixed slots, each a track with an identity that persists from block to
 * block and from call to call, hysteresis (a track opens after H hits and is held over B misses), a smoothed centre, the
 * exact channelizer phase_inc of that centre and a width class.  Slot s of source j is meant to be channelizer channel
 * j S + s: the host reads one block's slots and hands their phase_inc column to iqd_channelizer_set_channels.  Every quantity
 * is an integer and every step is fixed here, so results are exact; there are no floats.
 *
 *   input     the detector's two arrays for n_sources x n_blocks rows, in the spectrum's row order: rows_dev[n_sources][n_blocks]
 *             and det_dev[n_sources][n_blocks][K].  Of a row only n_found and the first D = min(n_found, K) records are read
 *             (of a record: first_bin, last_bin, peak_power, centroid_q8, which must be what the detector writes:
 *             first_bin <= last_bin < N, centroid_q8 < 256 N); the bytes past them may be anything.
 *   state     per source: the S slots as they stand after the last block, and next_id.  It persists across calls until
 *             iqd_track_reset (all slots all-zero bytes, next_id 0).  Sources are independent; the blocks of a source are
 *             processed in order.  One call of b1 + b2 blocks gives what a call of b1 blocks followed by one of b2 blocks gives.
 *   a block   G = gate_q8, H = open_hits, B = hold_blocks, A = alpha_q8; a slot is live iff state != 0, free iff state == 0.
 *     0 clear     every slot's flags become 0; a slot whose state is 0 (one that closed in the previous block) becomes
 *                 all-zero bytes.
 *     1 match     for detection i = 0 .. D - 1 in that order, c = det[i].centroid_q8: among the slots that are live, not yet
 *                 matched in this block and have |centre_q8 - c| <= G - centre_q8 as it stood when the block began - the one
 *                 with the least distance, on a tie the lowest slot index, is matched to detection i.  If there is none,
 *                 detection i is unmatched.
 *     2 update    every matched slot, from its detection: centre_q8 += ((c - centre_q8) A) >> 8, >> arithmetic (the floor
 *                 also for negative differences; |c - centre_q8| A < 2^27, and the result lies between the old centre and c,
 *                 so in [0, 256 N)); first_bin, last_bin, peak_power are the detection's;
 *                 max_width = max(max_width, last_bin - first_bin + 1); hits = min(hits + 1, 255); misses = 0; flag matched;
 *                 if state is 1 and hits >= H: state 2, flag opened.
 *     3 age       every slot that was live when the block began: age_blocks += 1 (mod 2^32).  If it was not matched:
 *                 misses += 1; a tentative slot (state 1) then becomes all-zero bytes at once; an active slot (state 2) with
 *                 misses > B gets state 0 and flag closed and keeps its other fields for this block's record only
 *                 (misses is stored mod 2^16: B = 65535 closes at a stored 0).
 *     4 allocate  the unmatched detections, in ascending i, take the lowest-index slots that were free when the block began
 *                 (after step 0); a slot freed or closed in this block is not available until the next block.
 *                 track_id = ++next_id (per source, mod 2^32); state 1 - or 2 with flag opened when H = 1; flags new and
 *                 matched; hits 1, misses 0, centre_q8 = c, age_blocks 0; first_bin, last_bin, peak_power the detection's,
 *                 max_width = last_bin - first_bin + 1.  A detection that finds no slot left counts in the block's n_unplaced.
 *     5 derive    every slot with track_id != 0:
 *                 phase_inc = (uint32)((centre_q8 - 128 N) 2^(24 - log2 N)) + inc_bias (mod 2^32): as a signed fraction of
 *                 2^32 exactly (centre_q8 / 256 - N / 2) / N of the wide rate, whatever the rate - what
 *                 iqd_channelizer_set_channels takes; |centre_q8 - 128 N| <= 2^18 at N = 2048 times 2^13, and so for every N
 *                 the product lies in [-2^31, 2^31).  width_class = the number of j with max_width >= class_edge[j].
 *   output    slots_dev[n_sources][n_blocks][S]: every slot as it stands after the block; blocks_dev[n_sources][n_blocks]:
 *             n_active and n_tentative after the block, the slots with flag opened | those with flag closed << 16, and the
 *             block's unplaced detections.  Both arrays are defined in full after a call.
 *   state, flags   state 0 free, 1 tentative, 2 active.  flags bit 0 matched this block, bit 1 new this block, bit 2 opened
 *             this block (became active), bit 3 closed this block.
 *   phase_inc iqd_track_phase_inc(N, centroid_q8, inc_bias): step 5's rule on the host, no GPU.  IQD_EINVAL: inc NULL, N outside
 *             the set, centroid_q8 >= 256 N.
 *   refusals  IQD_EINVAL with a message naming the argument, before anything is allocated or queued: a NULL pointer, a field
 *             outside its range, a non-zero reserved word; at run: n_blocks 0, n_sources n_blocks above 2^31 - 1, a NULL or
 *             misaligned device pointer; get_state: source >= n_sources.
 * rows_dev, det_dev, slots_dev, blocks_dev: device memory, 16-byte aligned.  The _device form is queued on the engine's stream
 * - straight behind the iqd_detect_run_device that writes its input - and returns once queued; the host form takes host
 * pointers and returns when done; iqd_track_get_state synchronises; iqd_track_reset is queued. */
typedef struct iqd_track_config {
    uint32_t n_sources;       /* >= 1 */
    uint32_t n_bins;          /* N: 64 ... 2048, the detector's */
    uint32_t max_detections;  /* K: 1 ... N / 2, the detector's */
    uint32_t n_slots;         /* S: 1 ... 64 */
    uint32_t gate_q8;         /* G: 0 ... 256 N - 1 */
    uint32_t open_hits;       /* H: 1 ... 255 */
    uint32_t hold_blocks;     /* B: 0 ... 65535 */
    uint32_t alpha_q8;        /* A: 1 ... 256 (256: the centre follows the detection) */
    uint32_t inc_bias;        /* added to every phase_inc mod 2^32 (e.g. the +64 kHz of "station + Fs/4") */
    uint32_t class_edge[3];   /* 1 <= e0 <= e1 <= e2 <= N + 1 (N + 1 is never reached) */
    uint32_t reserved[4];     /* 0 */
} iqd_track_config;
typedef struct iqd_track_slot {     /* 32 bytes */
    uint32_t track_id;              /* 0: free.  Per source, counted from 1 in order of allocation, mod 2^32 */
    uint8_t  state, flags, hits, width_class;
    uint16_t misses, max_width;
    uint32_t centre_q8, phase_inc;
    uint16_t first_bin, last_bin;
    uint32_t peak_power, age_blocks;
} iqd_track_slot;
typedef struct iqd_track_block {
    uint32_t n_active, n_tentative, n_opened_closed /* opened | closed << 16 */, n_unplaced;
} iqd_track_block;
#define IQD_TRACK_FREE 0
#define IQD_TRACK_TENTATIVE 1
#define IQD_TRACK_ACTIVE 2
#define IQD_TRACK_F_MATCHED 1
#define IQD_TRACK_F_NEW 2
#define IQD_TRACK_F_OPENED 4
#define IQD_TRACK_F_CLOSED 8
typedef struct iqd_track iqd_track_t;
int iqd_track_create(iqd_t *e, const iqd_track_config *cfg, iqd_track_t **out);
void iqd_track_destroy(iqd_track_t *t);   /* before its engine's iqd_destroy */
int iqd_track_reset(iqd_track_t *t);
int iqd_track_run_device(iqd_track_t *t, const iqd_detect_row *rows_dev, const iqd_detection *det_dev, size_t n_blocks,
                         iqd_track_slot *slots_dev, iqd_track_block *blocks_dev);
int iqd_track_run(iqd_track_t *t, const iqd_detect_row *rows, const iqd_detection *det, size_t n_blocks, iqd_track_slot *slots,
                  iqd_track_block *blocks);
int iqd_track_get_state(iqd_track_t *t, uint32_t source, iqd_track_slot *out /* [S] */);
int iqd_track_phase_inc(uint32_t n_bins, uint32_t centroid_q8, uint32_t inc_bias, uint32_t *inc);

/* Track-following channels: a channelizer channel may FOLLOW A SLOT of a track table - the slots array that
 * iqd_track_run_device writes, or any array of that layout - and is then cut, block by block, at the slot's phase_inc.  The
 * table is complete before the channelizer runs, so the retune stays on the device: iqd_track_run_device followed by the
 * channelizer call on the engine's stream needs no synchronise in between.  Anything not named here is the integer
 * channelizer's spec above.
 *
 *   blocks    a following channel's row of one call is n_blocks blocks of block_bytes bytes (block_bytes / 2 outputs, or
 *             block_bytes M wide bytes per source).  A spectrum block of 2 N F wide bytes is block_bytes = 2 N F / M; the
 *             caller chooses N, F and M so that this is a multiple of 64.
 *   length    a call with at least one follower needs bytes_per_source / M == n_blocks * block_bytes, whatever the engine's
 *             own block_bytes: the accept behind the channelizer sees ordinary rows.
 *   entry     channel c with source j (its set_channels source) and slot s reads, for block b, the table entry
 *             t = slots_dev[j][b - lag][s] - of it only state and phase_inc.  lag 1, block 0: the carry (below).
 *   cut       t.state >= min_state: the block is live and cut by exactly the integer spec with d_b = t.phase_inc - taps from
 *             d_b, the rotation P[(n d_b mod 2^32) >> 20] with absolute n, the channel's gain shift, the wide history as
 *             always.  Otherwise every byte of the block is 0x80: free slots, tentative ones under min_state 2, and a slot in
 *             its closing block (state 0 although track_id != 0).
 *   carry     per following channel, on the device: (live, d).  Every call with followers leaves it at the decision of its
 *             LAST table block, entry n_blocks - 1 of the channel's source and slot, whatever lag is.  With lag 1, block 0
 *             uses the carry, so one call of b1 + b2 blocks gives the bytes of a call of b1 followed by one of b2 with the
 *             table halves handed in by two set_track_table calls.  The carry is not live after create, after
 *             iqd_channelizer_reset, and for a channel that has just started to follow (or moved to another slot).
 *   settings  while a channel follows, its set_channels increment is kept but ignored (source and gain shift still apply);
 *             it is back in force at the next call after the channel stops.  reset keeps the flags and the table.  Several
 *             channels may follow one slot.  The table's memory is read when the kernel runs, in stream order; the table
 *             stays in force until it is replaced (NULL: no table).
 *   calls     track followers need no engine channel: they run under iqd_channelizer_run / _run_device and
 *             iqd_accept_wideband / _device, beside fixed channels; under the accept forms also beside scanner- and
 *             gain-following channels (which the run forms go on refusing).
 *   launches  one kernel launch per call whatever n_blocks for K <= 256; for longer prototypes two per run of blocks, the
 *             runs cut so that the per-(block, tile) operand scratch stays within 64 MiB (or one block's, where that is more).
 *   refusals  IQD_EINVAL before anything is queued, the message naming the reason, the stream intact afterwards.
 *             set_track_table: a non-zero reserved word; n_slots outside 1..64; n_blocks 0; block_bytes 0 or no multiple of
 *             64; lag > 1; min_state not 1 or 2; slots_dev NULL or not 16-byte aligned.  follow_tracks: a slot < -1 or > 63;
 *             a bad channel range; a slot >= 0 on a fractional channelizer or on signed captures, or on a channel that follows
 *             its scanner or its gain - and follow_scanner / follow_gain(..., 1) on a track follower.  A call with followers:
 *             no table set; a follower's slot >= the table's n_slots; the length rule violated.  iqd_channelizer_survey*
 *             while any channel follows tracks.
 * iqd_channelizer_follow_tracks: slot[i] >= 0: channel first + i follows that slot of ITS source's table row; -1, or
 *             slot == NULL: it stops following.
 * iqd_channelizer_track_window_outputs (host only, no GPU): iqd_channelizer_window_outputs for a track follower's window,
 *             which shares its LDS with the prototype: t with 2 (t M + Kp) <= 32768 - 2048, cut to a multiple of 64 and to 1024. */
typedef struct iqd_track_follow {
    const iqd_track_slot *slots_dev;  /* [n_sources][n_blocks][n_slots], as iqd_track_run_device writes it; 16-byte aligned */
    uint32_t n_slots;                 /* S of the table, 1 ... 64 */
    uint32_t n_blocks;                /* table blocks per source, >= 1 */
    uint32_t block_bytes;             /* row bytes (output bytes of one channel) that one table block covers: a multiple of 64 */
    uint32_t lag;                     /* 0: block b is cut at table block b; 1: at table block b - 1 (block 0: the carry) */
    uint32_t min_state;               /* IQD_TRACK_TENTATIVE (1) or IQD_TRACK_ACTIVE (2) */
    uint32_t reserved[3];             /* 0 */
} iqd_track_follow;
int iqd_channelizer_set_track_table(iqd_channelizer_t *z, const iqd_track_follow *t);   /* NULL: no table */
int iqd_channelizer_follow_tracks(iqd_channelizer_t *z, uint32_t first, uint32_t n, const int32_t *slot);
uint32_t iqd_channelizer_track_window_outputs(uint32_t decimation, uint32_t n_taps);

/* Band track measurements: what a track IS - for every (source, block, slot) the power over the noise floor, the occupied
 * bandwidth in the ITU sense (the band that holds all but beta of the power at each end), the share of the power that sits
 * in the carrier, and from those a mode hint.  A stateless object queued on the engine's stream straight behind
 * iqd_track_run_device; it reads the spectrum's power rows again, which the tracker never does.  Every quantity is an unsigned
 * integer and every step is fixed here, so results are exact; there are no floats.
 *
 *   input     power_dev[n_sources][n_blocks][N] uint32 (iqd_spectrum_run_device's, any values up to 2^32 - 1 are legal);
 *             rows_dev[n_sources][n_blocks] (iqd_detect_run_device's; only floor is read);
 *             slots_dev[n_sources][n_blocks][S] (iqd_track_run_device's; only track_id, state, first_bin and last_bin are
 *             read, and they must be what the tracker writes: first_bin <= last_bin < N).
 *   config    N = n_bins 64 ... 2048, a power of two; S = n_slots 1 ... 64; d = dc_guard 0 ... N / 4 (the detector's meaning);
 *             m = margin 0 ... 64; beta = obw_tail_q16 0 ... 32767; c = carrier_half 0 ... 8; min_sum any; carrier_min_q8
 *             0 ... 256; wide_bins 1 ... N + 1; n_sources >= 1; reserved 0.
 *   entry     (j, b, s): t = slots[j][b][s], p = power[j][b], f = rows[j][b].floor.
 *   measured  iff t.state != 0.  A free slot, and a slot in its closing block (state 0 with track_id still set), gives 32
 *             zero bytes.
 *   excess    e[k] = p[k] > f ? p[k] - f : 0, and e[k] = 0 for the guard bins N / 2 - d < k < N / 2 + d.
 *   window    lo = max(first_bin - m, 0), hi = min(last_bin + m, N - 1); everything below is over lo .. hi.
 *   sums      sum_excess E = sum e (uint64; below 2^32 x 2^11 = 2^43); n_over = the number of bins with e > 0;
 *             peak_excess = max e; peak_bin = the lowest bin that has it.
 *   empty     E = 0: flags = IQD_MEASURE_F_EMPTY, track_id stays, every other field is 0.
 *   weak      E < min_sum: flag IQD_MEASURE_F_WEAK; the fields are computed all the same; hint = IQD_HINT_NONE.
 *   centroid  centroid_q8 = floor(256 sum k e[k] / E), k the absolute bin: sum k e < 2^11 x 2^43 = 2^54, its 256-fold < 2^62.
 *   obw       L(k) = sum over lo .. k of e, R(k) = sum over k .. hi of e.  obw_lo = the least k with 65536 L(k) > beta E,
 *             obw_hi = the greatest k with 65536 R(k) > beta E; both products are below 2^16 x 2^43 = 2^59.  obw_lo <= obw_hi
 *             always: with a = obw_lo, L(a - 1) <= beta E / 65536 (or a = lo and L(a - 1) = 0), so
 *             65536 R(a) = 65536 (E - L(a - 1)) >= (65536 - beta) E > beta E for beta <= 32767 and E > 0: a passes obw_hi's test.
 *   carrier   C = sum e over max(lo, peak_bin - c) .. min(hi, peak_bin + c); carrier_q8 = floor(256 C / E), 0 ... 256.
 *   hint      of a measured entry that is neither weak nor empty: IQD_HINT_WIDE if obw_hi - obw_lo + 1 >= wide_bins, otherwise
 *             IQD_HINT_CARRIER if carrier_q8 >= carrier_min_q8, otherwise IQD_HINT_NARROW.
 *   limits    the hint is a hint; the measurements are the product.  It sees one block's power and nothing else: an
 *             unmodulated FM carrier (a pause in speech) looks like CARRIER; a sideband signal has no carrier at all and looks
 *             like NARROW; a strong neighbour inside the margin is measured with the track.  Nothing is smoothed across
 *             blocks; the host decides what to do with a block's hints.
 *   output    meas_dev[n_sources][n_blocks][S], defined in full after every call.
 *   refusals  IQD_EINVAL with a message naming the argument, before anything is allocated or queued, the stream intact: a
 *             NULL pointer, a field outside its range, a non-zero reserved word; at run: n_blocks 0, n_sources n_blocks above
 *             2^31 - 1, a device pointer that is NULL or not 16-byte aligned.
 * The _device form is queued and returns once queued; the host form takes host pointers and returns when done. */
typedef struct iqd_measure_config {
    uint32_t n_sources;       /* >= 1 */
    uint32_t n_bins;          /* N: 64 ... 2048, a power of two */
    uint32_t n_slots;         /* S: 1 ... 64, the tracker's */
    uint32_t dc_guard;        /* d: 0 ... N / 4, the detector's */
    uint32_t margin;          /* m: 0 ... 64 bins added on each side of the track's run */
    uint32_t obw_tail_q16;    /* beta: 0 ... 32767, the share of the power left outside at EACH end (328: 0.5 %) */
    uint32_t carrier_half;    /* c: 0 ... 8 bins on each side of the peak that count as carrier */
    uint32_t min_sum;         /* below this sum of excess power a track is weak and gets no hint */
    uint32_t carrier_min_q8;  /* 0 ... 256 */
    uint32_t wide_bins;       /* 1 ... N + 1 (N + 1 is never reached) */
    uint32_t reserved[2];     /* 0 */
} iqd_measure_config;
typedef struct iqd_track_measure {   /* 32 bytes */
    uint32_t track_id;
    uint16_t obw_lo, obw_hi, peak_bin;
    uint8_t  flags, hint;
    uint32_t peak_excess, centroid_q8;
    uint16_t carrier_q8, n_over;
    uint64_t sum_excess;
} iqd_track_measure;
#define IQD_MEASURE_F_EMPTY 1
#define IQD_MEASURE_F_WEAK 2
#define IQD_HINT_NONE 0
#define IQD_HINT_CARRIER 1
#define IQD_HINT_NARROW 2
#define IQD_HINT_WIDE 3
typedef struct iqd_measure iqd_measure_t;
int iqd_measure_create(iqd_t *e, const iqd_measure_config *cfg, iqd_measure_t **out);
void iqd_measure_destroy(iqd_measure_t *m);   /* before its engine's iqd_destroy */
int iqd_measure_run_device(iqd_measure_t *m, const uint32_t *power_dev, const iqd_detect_row *rows_dev, const iqd_track_slot *slots_dev,
                           size_t n_blocks, iqd_track_measure *meas_dev);
int iqd_measure_run(iqd_measure_t *m, const uint32_t *power, const iqd_detect_row *rows, const iqd_track_slot *slots, size_t n_blocks,
                    iqd_track_measure *meas);

/* Band track log: what the band DID - a running summary of every (source, slot) over its track's whole life, across blocks
 * and calls, a mode hint voted over every measured block so far, and one compact event record when a track ends: when, where,
 * how wide, what kind.  A stateful object queued on the engine's stream straight behind iqd_measure_run_device; capture ->
 * spectrum -> detector -> tracker -> measurements -> log stays one stream and one synchronise, and the host reads a handful
 * of 64-byte events instead of whole tables.  Integers only; every step is fixed here, so results are exact.
 *
 *   input     slots_dev[n_sources][n_blocks][S] (iqd_track_run_device's; of a slot only track_id, state, width_class and
 *             centre_q8 are read); meas_dev[n_sources][n_blocks][S] (iqd_measure_run_device's).
 *   config    S = n_slots 1 ... 64; E = max_events 1 ... 65536; min_active 1 ... 65535; vote_min 1 ... 65535; n_sources >= 1;
 *             reserved 0.
 *   state     per source: a uint64 block index g - the blocks of the source seen since create / reset - and S summaries.  It
 *             persists across calls until iqd_tracklog_reset (all zero).  Sources are independent; the blocks of a source are
 *             processed in order.
 *   a block   per slot: t = the table's slot, m = its measurement record, st = the slot's summary.  st.flags becomes 0 first.
 *     0 vanished    st.track_id != 0 and t.track_id != st.track_id: the track ends LOST.  It is an event - st as it stands, with
 *                   flags = IQD_TLOG_F_LOST - if st.n_active >= min_active; otherwise it counts in n_short.  st becomes
 *                   all-zero bytes.  This covers a tracker reset between calls, a tentative slot dropped at its first miss,
 *                   and any foreign table.
 *     1 start       t.track_id != 0 and st.track_id == 0: st.track_id = t.track_id, first_block = g, flag NEW,
 *                   obw_lo_min = 0xffff (and is shown as such until a block votes).
 *                   After steps 0 and 1 st.track_id == t.track_id.  A table slot with track_id 0 is free whatever its state
 *                   says: steps 2 to 4 apply only where st.track_id != 0 (the tracker never writes such a slot; a foreign
 *                   table could, and a summary must not gather blocks under no id).
 *     2 accumulate  if t.state != 0: n_blocks += 1; state = t.state; width_class = t.width_class.  If t.state == 2:
 *                   n_active += 1, sum_centre_q8 += t.centre_q8.  The block VOTES iff m.track_id == t.track_id and
 *                   m.flags == 0 (neither empty nor weak); then n_measured += 1, sum_excess += m.sum_excess,
 *                   peak_excess = max(peak_excess, m.peak_excess), obw_lo_min = min(obw_lo_min, m.obw_lo),
 *                   obw_hi_max = max(obw_hi_max, m.obw_hi), and if m.hint is 1, 2 or 3: votes[m.hint - 1] += 1 (any other
 *                   hint value adds to no vote).  Counters are mod 2^32.
 *     3 decide      V = votes[0] + votes[1] + votes[2] (mod 2^32 like the counters).  mode_hint = 0 while V < vote_min;
 *                   otherwise the hint with the most votes, ties to the lowest hint.  Flag MODE_CHANGED if it differs from
 *                   the value st had before this block (0 -> x included).
 *     4 close       t.state == 0 (the tracker's closing block: state 0 with the id still set): flag CLOSED, state = 0.  It is
 *                   an event if n_active >= min_active; otherwise it counts in n_short.  The block's output shows this final
 *                   record; afterwards st is all-zero bytes.
 *     5 advance     g += 1, once per block of the source.
 *   output    all three arrays are defined in full after every call.
 *             summary_dev[n_sources][n_blocks][S]: st as it stands after the block (before step 4's zeroing); a free slot is
 *             64 zero bytes.
 *             events_dev[n_sources][E]: the call's events of that source, ordered by block and within a block by ascending
 *             slot (a slot ends at most one track that is an event per block: a track that starts and closes in one block
 *             has n_active 0 < min_active).  An event is the summary as it stood when the track ended.  Entries from n_stored
 *             on are zero bytes.
 *             counts_dev[n_sources]: n_events counts all events of the call, n_stored = min(n_events, E), n_lost those of
 *             n_events that are LOST, n_short the ended tracks that were no event (mod 2^32; 2^32 events need 2^32 table
 *             entries of 128 bytes in and out, more than a device holds).
 *   calls     a call of b1 + b2 blocks gives the summaries of a call of b1 followed by one of b2; its events are the two
 *             calls' events concatenated and its counts their sums, as long as E is not exceeded.
 *   get_state the source's S summaries as they stand after the last block (flags included; a track closed in that block is
 *             zero bytes already) and g.  Synchronises.
 *   mean      iqd_tracklog_mean_centre(sum_centre_q8, n_active): floor(sum / n) on the host, no GPU; with
 *             iqd_track_phase_inc the track's mean tuning.  IQD_EINVAL: n_active 0, centre_q8 NULL, or a quotient of 2^32 or more (no
 *             sum of centres below 2^19 gives one).
 *   bounds    centre_q8 < 2^19, so sum_centre_q8 stays below 2^51 over 2^32 blocks.  m.sum_excess < 2^43 per block: the uint64
 *             sum_excess wraps only after 2^21 voting blocks of saturated rows, hence mod 2^64.
 *   refusals  IQD_EINVAL with a message naming the argument, before anything is allocated or queued, the stream intact: a
 *             NULL pointer, a field outside its range, a non-zero reserved word; at run: n_blocks 0, n_sources n_blocks above
 *             2^31 - 1, a device pointer that is NULL or not 16-byte aligned; get_state: source >= n_sources.
 * The _device form is queued and returns once queued; the host form takes host pointers and returns when done;
 * iqd_tracklog_reset is queued. */
typedef struct iqd_tracklog_config {
    uint32_t n_sources;   /* >= 1 */
    uint32_t n_slots;     /* S: 1 ... 64, the tracker's */
    uint32_t max_events;  /* E: 1 ... 65536 event records per source and call */
    uint32_t min_active;  /* 1 ... 65535: a track that ends with fewer active blocks is not an event */
    uint32_t vote_min;    /* 1 ... 65535: votes needed before a mode is decided */
    uint32_t reserved[3]; /* 0 */
} iqd_tracklog_config;
typedef struct iqd_track_summary {       /* 64 bytes, naturally aligned */
    uint32_t track_id;                   /* 0: free */
    uint8_t  state, flags, mode_hint, width_class;
    uint64_t first_block;                /* the source's block index g at which the log first saw the track */
    uint32_t n_blocks, n_active;         /* blocks seen live (state != 0) / active (state 2) */
    uint32_t n_measured, votes[3];       /* blocks that voted; votes for IQD_HINT_CARRIER / NARROW / WIDE */
    uint64_t sum_centre_q8;              /* sum of the slot's centre_q8 over its active blocks */
    uint64_t sum_excess;                 /* sum of sum_excess over the blocks that voted, mod 2^64 */
    uint32_t peak_excess;                /* max over the blocks that voted */
    uint16_t obw_lo_min, obw_hi_max;     /* extremes over the blocks that voted */
} iqd_track_summary;
#define IQD_TLOG_F_NEW 1           /* first block of this summary */
#define IQD_TLOG_F_MODE_CHANGED 2  /* mode_hint differs from the previous block's (0 -> x included) */
#define IQD_TLOG_F_CLOSED 4        /* the tracker closed the track in this block */
#define IQD_TLOG_F_LOST 8          /* events only: the track vanished from its slot without a closing block */
typedef struct iqd_tracklog_counts { uint32_t n_events, n_stored, n_short, n_lost; } iqd_tracklog_counts;
typedef struct iqd_tracklog iqd_tracklog_t;
int iqd_tracklog_create(iqd_t *e, const iqd_tracklog_config *cfg, iqd_tracklog_t **out);
void iqd_tracklog_destroy(iqd_tracklog_t *t);   /* before its engine's iqd_destroy */
int iqd_tracklog_reset(iqd_tracklog_t *t);
int iqd_tracklog_run_device(iqd_tracklog_t *t, const iqd_track_slot *slots_dev, const iqd_track_measure *meas_dev, size_t n_blocks,
                            iqd_track_summary *summary_dev, iqd_track_summary *events_dev, iqd_tracklog_counts *counts_dev);
int iqd_tracklog_run(iqd_tracklog_t *t, const iqd_track_slot *slots, const iqd_track_measure *meas, size_t n_blocks, iqd_track_summary *summary,
                     iqd_track_summary *events, iqd_tracklog_counts *counts);
int iqd_tracklog_get_state(iqd_tracklog_t *t, uint32_t source, iqd_track_summary *out /* [S] */, uint64_t *next_block /* g */);
int iqd_tracklog_mean_centre(uint64_t sum_centre_q8, uint32_t n_active, uint32_t *centre_q8);

/* PCM of several engines (one per GPU, one host process each or all in one) into one place over RCCL / xGMI.  The data
 * path itself has no collective - channels are independent, every GPU demodulates its own - this only
 * delivers the audio, 1/32 of the input volume, to one rank.  The reference has no counterpart (one dongle, one
 * process); the sink it stands in front of is radioApp.cc:103-111.
 *   iqd_gather_unique_id   the root makes an id; the host passes it to the other ranks by any means of its own
 *   iqd_gather_create      every rank, with its own engine (its GPU current), the id, its rank, the world size
 *   iqd_gather_pcm         every rank: its bytes_per_rank[rank] bytes at send_dev go to row `rank` of recv_dev on the
 *                          root (rows row_stride bytes apart; recv_dev is ignored elsewhere).  Queued on the engine's
 *                          stream behind the accept that produced the PCM; the next accept queues behind it.
 * librccl.so is loaded when the first of these is called.  IQD_ENODEV: no RCCL on this host. */
#define IQD_GATHER_ID_BYTES 128
typedef struct iqd_gather iqd_gather_t;
int iqd_gather_unique_id(uint8_t *id128);
int iqd_gather_create(iqd_t *e, const uint8_t *id128, uint32_t rank, uint32_t world, uint32_t root, iqd_gather_t **out);
int iqd_gather_pcm(iqd_gather_t *g, const void *send_dev, const size_t *bytes_per_rank, void *recv_dev, size_t row_stride);
void iqd_gather_destroy(iqd_gather_t *g);
/* RCCL's version code, the rank count the communicator reports (ncclCommCount; g may be NULL: 0), and whether an RCCL the
 * process had loaded already (a torch host's) was reused instead of opening a second copy.  Any pointer may be NULL. */
int iqd_gather_info(iqd_gather_t *g, int *rccl_version, int *comm_ranks, int *library_reused);

/* Small device-memory helpers so that non-HIP hosts (ctypes, cgo, JNI) can stage
 * device-resident buffers for iqd_accept_iq_device without linking the HIP runtime. */
int iqd_dev_alloc(iqd_t *e, size_t bytes, void **out);
int iqd_dev_free(iqd_t *e, void *p);
int iqd_dev_upload(iqd_t *e, void *dst_dev, const void *src_host, size_t bytes);
int iqd_dev_download(iqd_t *e, void *dst_host, const void *src_dev, size_t bytes);
/* Page-locked host memory for iqd_accept_iq: with it the uploads are true DMA and, for calls of 64 MiB and more,
 * overlap the kernels (the call is cut into ~32 MiB slices through two device staging sets; this stands in for
 * the reference's ring of receive buffers, DataConsumer.cc:220-352).  Pageable buffers work too, more slowly. */
int iqd_host_alloc(iqd_t *e, size_t bytes, void **out);
int iqd_host_free(iqd_t *e, void *p);
/* Fills dst_dev with `total` bytes by repeating the first `period` bytes already there. */
int iqd_dev_tile(iqd_t *e, void *dst_dev, size_t period, size_t total);
void *iqd_stream(iqd_t *e); /* the engine's hipStream_t */
int iqd_device_count(void); /* HIP devices this process can see (0 without a usable runtime): what iqd_config::device may name */
int iqd_get_device(iqd_t *e, int *device); /* the HIP device ordinal the engine lives on (iqd_config::device resolved) */
/* Diagnostic builds (-DIQD_STAMPS) only: cycle sums per kernel phase; zeros otherwise. */
int iqd_debug_stamps(iqd_t *e, unsigned long long *out16);
int iqd_debug_stamps_ext(iqd_t *e, unsigned long long *out, uint32_t n);   /* the first n <= 32768 of them (IQD_ST_TIMING / IQD_ST_WAITSTAT / IQD_ST_TRACE builds) */

#ifdef __cplusplus
}
#endif
#endif /* IQDEMOD_H */
