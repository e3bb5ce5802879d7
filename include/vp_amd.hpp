// vp_amd.hpp -- header-only C++ adapter over the C ABI (vp_amd.h).
//
// `vp::BatchVocoderProcessor` mirrors the call surface of the reference's
// VocoderAudioProcessor (PluginProcessor.h:24-80) for a batch of streams, so host code written
// against the plugin reads the same:
//
//     vp::BatchVocoderProcessor proc(/*device*/ 0);
//     proc.setParameter("lpcVoice", 24);              // treeState.getRawParameterValue(id)->store(v)
//     proc.prepareToPlay(44100.0, 1024, /*streams*/ 256);
//     proc.processBlock(io);                           // float io[streams][3][N], in place
//
// and a `vp::BufferView` with the MyBuffer getters (MyBuffer.h:37-43) for code that sized its own
// buffers from them.  Errors become exceptions carrying the C status code.
#pragma once

#include <condition_variable>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "vp_amd.h"

namespace vp {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

namespace detail {
// what the streaming classes do with a return code (their handles keep no message of their own)
inline void check(int rc, const std::string &what)
{
    if (rc != VP_OK) throw Error(rc, what + ": " + vp_error_string(rc));
}
}  // namespace detail

// MyBuffer.h:37-43
struct BufferView {
    int geom[12];
    int getSamplesPerBlock() const { return geom[0]; }
    int getLatency() const { return geom[7]; }
    int getIdxMax() const { return geom[7] + geom[0]; }
    int getSamplesToKeep() const { return geom[6]; }
    int getInSize() const { return geom[8]; }
    int getNumOutChannels() const { return 2; }
};

class BatchVocoderProcessor {
public:
    explicit BatchVocoderProcessor(int device = 0)
    {
        check(vp_create(device, &h_), "vp_create");                 // createPluginFilter()
        vp_default_params(&p_);
    }
    ~BatchVocoderProcessor() { if (h_) vp_destroy(h_); }
    BatchVocoderProcessor(const BatchVocoderProcessor &) = delete;
    BatchVocoderProcessor &operator=(const BatchVocoderProcessor &) = delete;

    // ids and ranges of createParameterLayout() (PluginProcessor.cpp:37-73)
    void setParameter(const char *id, float v)
    {
        vp_params q = p_;
        if (!std::strcmp(id, "gainPitch")) q.gainPitch = v;
        else if (!std::strcmp(id, "gainVoice")) q.gainVoice = v;
        else if (!std::strcmp(id, "gainSynth")) q.gainSynth = v;
        else if (!std::strcmp(id, "gainVoc")) q.gainVoc = v;
        else if (!std::strcmp(id, "lpcVoice")) q.lpcVoice = (int)v;
        else if (!std::strcmp(id, "lpcPitch")) q.lpcPitch = (int)v;
        else if (!std::strcmp(id, "lpcSynth")) q.lpcSynth = (int)v;
        else if (!std::strcmp(id, "keyPitch")) q.keyPitch = (int)v;
        else if (!std::strcmp(id, "pitchBool")) q.pitchBool = (int)v;
        else if (!std::strcmp(id, "vocBool")) q.vocBool = (int)v;
        else throw Error(VP_ERR_INVALID_ARG, std::string("unknown parameter ") + id);
        check(vp_set_params(h_, &q), id);
        p_ = q;
    }
    const vp_params &parameters() const { return p_; }
    // one stream's own treeState value (after prepare; every parameter but lpcPitch, which is read at prepare)
    // extension: fixed interval (+-12 semitones) instead of the key's nearest note; stream = -1: all streams
    void setPitchShift(double semitones, bool on = true, int stream = -1) { check(vp_set_pitch_shift(h_, stream, on ? 1 : 0, semitones), "setPitchShift"); }
    void setStreamParameter(int stream, const char *id, float v)
    {
        vp_params q;
        check(vp_get_stream_params(h_, stream, &q), "getStreamParams");
        if (!std::strcmp(id, "gainPitch")) q.gainPitch = v;
        else if (!std::strcmp(id, "gainVoice")) q.gainVoice = v;
        else if (!std::strcmp(id, "gainSynth")) q.gainSynth = v;
        else if (!std::strcmp(id, "gainVoc")) q.gainVoc = v;
        else if (!std::strcmp(id, "lpcVoice")) q.lpcVoice = (int)v;
        else if (!std::strcmp(id, "lpcSynth")) q.lpcSynth = (int)v;
        else if (!std::strcmp(id, "keyPitch")) q.keyPitch = (int)v;
        else if (!std::strcmp(id, "pitchBool")) q.pitchBool = (int)v;     // PluginProcessor.cpp:214-221: each instance has its own
        else if (!std::strcmp(id, "vocBool")) q.vocBool = (int)v;
        else throw Error(VP_ERR_INVALID_ARG, std::string("not a per-stream parameter: ") + id);
        check(vp_set_stream_params(h_, stream, &q), id);
    }

    // which implementation runs VocoderProcess::process (VP_VOC_AUTO / VP_VOC_WORKGROUP / VP_VOC_BATCHED; same results)
    void setVocoderPath(int path) { check(vp_set_vocoder_path(h_, path), "setVocoderPath"); }
    // VP_IIR_FAST: pitch corrector beside the vocoder pipeline's tail instead of behind it: 0 / 1 / VP_OVERLAP_AUTO (the default)
    void setOverlap(int mode) { check(vp_set_overlap(h_, mode), "setOverlap"); }
    void setIirMode(int mode) { check(vp_set_iir_mode(h_, mode), "setIirMode"); }
    void setYinMode(int mode) { check(vp_set_yin_mode(h_, mode), "setYinMode"); }

    void prepareToPlay(double sampleRate, int samplesPerBlock, int nStreams)      // PluginProcessor.cpp:144
    {
        check(vp_prepare_to_play(h_, sampleRate, samplesPerBlock, nStreams), "prepareToPlay");
    }
    void prepareExplicit(double sampleRate, int samplesPerBlock, int nStreams, int frameLenPitch, int hopPitch,
                         int wlenVoc, int hopVoc)                                   // :172-181 with explicit sizes
    {
        check(vp_prepare_explicit(h_, sampleRate, samplesPerBlock, nStreams, frameLenPitch, hopPitch, wlenVoc, hopVoc),
              "prepareExplicit");
    }
    // processBlock(AudioBuffer<float>&, MidiBuffer&) (:203): io [streams][3][N] in place, host memory
    void processBlock(float *io) { check(vp_process_block_inplace(h_, io), "processBlock"); }
    void processBlock(const float *in, float *out) { check(vp_process_block(h_, in, out), "processBlock"); }
    // what AudioBuffer<float> holds: one pointer per channel (getReadPointer / getWritePointer), row (s, ch) = in[s * nIn + ch];
    // nIn 1 or 3, nOut 2 or 3; a null input is silence (MyBuffer.cpp:93-102), a null output is not written, out may alias in
    void processBlock(const float *const *in, int nIn, float *const *out, int nOut)
    {
        check(vp_process_block_channels(h_, in, nIn, out, nOut), "processBlock");
    }
    // the same with DEVICE tables of device rows, asynchronous on `hipStream`; rows of nBlocks * N samples in the second form
    void processBlockChannelsDevice(const float *const *dIn, int nIn, float *const *dOut, int nOut, void *hipStream = nullptr)
    {
        check(vp_process_block_channels_device(h_, dIn, nIn, dOut, nOut, hipStream), "processBlockChannelsDevice");
    }
    void processBlocksChannelsDevice(const float *const *dIn, int nIn, float *const *dOut, int nOut, int nBlocks, void *hipStream = nullptr)
    {
        check(vp_process_blocks_channels_device(h_, dIn, nIn, dOut, nOut, nBlocks, hipStream), "processBlocksChannelsDevice");
    }
    // device-resident, asynchronous on `hipStream`
    void processBlockDevice(const float *dIn, float *dOut, void *hipStream = nullptr)
    {
        check(vp_process_block_device(h_, dIn, dOut, hipStream), "processBlockDevice");
    }
    // buffers without the side-chain bus: voice [streams][N] (null side-chain pointers -> zeros, MyBuffer.cpp:93-102)
    void processBlockMono(const float *voice, float *out) { check(vp_process_block_mono(h_, voice, out), "processBlockMono"); }
    void processBlockMonoDevice(const float *dVoice, float *dOut, void *hipStream = nullptr)
    {
        check(vp_process_block_mono_device(h_, dVoice, dOut, hipStream), "processBlockMonoDevice");
    }
    void processBlocksMonoDevice(const float *dVoice, float *dOut, int nBlocks, void *hipStream = nullptr)
    {
        check(vp_process_blocks_mono_device(h_, dVoice, dOut, nBlocks, hipStream), "processBlocksMonoDevice");
    }
    // nBlocks consecutive processBlock() calls at once: dIn [nBlocks][streams][3][N], dOut [nBlocks][streams][2][N]
    void processBlocksDevice(const float *dIn, float *dOut, int nBlocks, void *hipStream = nullptr)
    {
        check(vp_process_blocks_device(h_, dIn, dOut, nBlocks, hipStream), "processBlocksDevice");
    }
    // sizes the multi-block scratch and staging for calls of up to nBlocks blocks: the process calls never allocate (vp_amd.h)
    void reserveBlocks(int nBlocks) { check(vp_reserve_blocks(h_, nBlocks), "reserveBlocks"); }
    // the same from host memory (upload, the blocks, download, in groups of the reserved size)
    void processBlocks(const float *in, float *out, int nBlocks) { check(vp_process_blocks(h_, in, out, nBlocks), "processBlocks"); }
    int getLatencySamples() const { return vp_get_latency(h_); }                   // :183
    // waits for everything launched on the handle's device and reports what poisoned the handle, if anything (VP_ERR_TIMEOUT: a
    // kernel's bounded wait ran out): the call a host makes before it trusts what the device-pointer entry points produced
    void synchronize() { check(vp_synchronize(h_), "synchronize"); }
    BufferView bufferView() const
    {
        BufferView v;
        check(vp_get_geometry(h_, v.geom), "geometry");
        return v;
    }
    vp_handle *handle() { return h_; }

private:
    void check(int rc, const std::string &what) const
    {
        if (rc != VP_OK)
            throw Error(rc, what + ": " + vp_error_string(rc) + (h_ ? std::string(" (") + vp_last_error(h_) + ")" : ""));
    }
    vp_handle *h_ = nullptr;
    vp_params p_;
};

// ------------------------------------------------------------------------------------------------
// vp::ShardedBatchProcessor -- the batch split over several GPUs of one node from ONE host process.
//
// The reference's ownership model is one plugin instance per stream (PluginProcessor.h:69-73: every instance owns its MyBuffer and
// its two processes); streams share nothing, so a batch shards by stream with no exchange between the shards.  This is the C++-level
// form of that split: one handle (a BatchVocoderProcessor) per device in `devices`, shard g owning the contiguous streams
// shardRange(g) -- the same ranges as vocoderproject_amd/dist.py's shard_range (sizes differ by at most one) --, and one persistent
// worker thread per shard that drives its handle (the C ABI's threading contract: one caller thread per handle), so the shards'
// uploads, kernels and downloads run side by side.  A call returns when every shard has.  No RCCL is involved: within one
// process the host buffers are simply addressed per shard.  (Several entries of `devices` may name the same GPU: that is how the
// helper is tested on a one-GPU box, against one handle, bit for bit.)
class ShardedBatchProcessor {
public:
    explicit ShardedBatchProcessor(const std::vector<int> &devices)
    {
        if (devices.empty()) throw Error(VP_ERR_INVALID_ARG, "ShardedBatchProcessor: no devices");
        for (int dev : devices) shards_.emplace_back(new Shard(dev));
    }
    ~ShardedBatchProcessor() = default;                                          // (every shard stops and joins its own worker)
    ShardedBatchProcessor(const ShardedBatchProcessor &) = delete;
    ShardedBatchProcessor &operator=(const ShardedBatchProcessor &) = delete;

    int numShards() const { return (int)shards_.size(); }
    // [first, first + count) of the batch's streams that shard g owns
    std::pair<int, int> shardRange(int g) const
    {
        const int G = numShards(), base = nStreams_ / G, rem = nStreams_ % G;
        return {g * base + (g < rem ? g : rem), base + (g < rem ? 1 : 0)};
    }
    BatchVocoderProcessor &shard(int g) { return shards_[g]->proc; }

    void setParameter(const char *id, float v) { for (auto &sh : shards_) sh->proc.setParameter(id, v); }
    void setStreamParameter(int stream, const char *id, float v)
    {
        const auto o = owner(stream);
        shards_[o.first]->proc.setStreamParameter(o.second, id, v);
    }
    void setPitchShift(double semitones, bool on = true, int stream = -1)
    {
        if (stream < 0) { for (auto &sh : shards_) sh->proc.setPitchShift(semitones, on, -1); return; }
        const auto o = owner(stream);
        shards_[o.first]->proc.setPitchShift(semitones, on, o.second);
    }
    void prepareToPlay(double sampleRate, int samplesPerBlock, int nStreams)      // PluginProcessor.cpp:144, per shard
    {
        if (nStreams < numShards()) throw Error(VP_ERR_INVALID_ARG, "ShardedBatchProcessor: fewer streams than shards");
        nStreams_ = nStreams; N_ = samplesPerBlock;
        run([&](int g, Shard &sh) { sh.proc.prepareToPlay(sampleRate, samplesPerBlock, shardRange(g).second); });
    }
    void prepareExplicit(double sampleRate, int samplesPerBlock, int nStreams, int frameLenPitch, int hopPitch, int wlenVoc, int hopVoc)
    {
        if (nStreams < numShards()) throw Error(VP_ERR_INVALID_ARG, "ShardedBatchProcessor: fewer streams than shards");
        nStreams_ = nStreams; N_ = samplesPerBlock;
        run([&](int g, Shard &sh) { sh.proc.prepareExplicit(sampleRate, samplesPerBlock, shardRange(g).second, frameLenPitch, hopPitch, wlenVoc, hopVoc); });
    }
    // processBlock (:203) on the whole batch: in [streams][3][N] -> out [streams][2][N], host memory; every shard works on its rows
    void processBlock(const float *in, float *out)
    {
        run([&](int g, Shard &sh) { const int lo = shardRange(g).first; sh.proc.processBlock(in + (size_t)lo * 3 * N_, out + (size_t)lo * 2 * N_); });
    }
    void processBlock(float *io)                                                  // in place: [streams][3][N]
    {
        run([&](int g, Shard &sh) { sh.proc.processBlock(io + (size_t)shardRange(g).first * 3 * N_); });
    }
    void processBlockMono(const float *voice, float *out)                         // voice [streams][N] -> out [streams][2][N]
    {
        run([&](int g, Shard &sh) { const int lo = shardRange(g).first; sh.proc.processBlockMono(voice + (size_t)lo * N_, out + (size_t)lo * 2 * N_); });
    }
    // channel pointers for the whole batch, host memory: a shard's tables are the caller's, offset to its first stream (no copy)
    void processBlock(const float *const *in, int nIn, float *const *out, int nOut)
    {
        run([&](int g, Shard &sh) { const int lo = shardRange(g).first; sh.proc.processBlock(in + (size_t)lo * nIn, nIn, out + (size_t)lo * nOut, nOut); });
    }
    int getLatencySamples() const { return shards_[0]->proc.getLatencySamples(); }

    // ---- device-resident, asynchronous forms (the rate bench.py reports is reached with inputs resident in HBM) -----------------------
    // Every shard's buffers live on ITS device: dIn[g] = [shardRange(g).second][3][N] floats on device devices[g], dOut[g] likewise
    // with 2 channels; hipStreams[g] (optional) a stream of that device.  The calls ENQUEUE shard g's kernels from shard g's worker
    // thread -- side by side, the handles' host work included -- and return when all are enqueued, not when they have run:
    // synchronize() (or the caller's own stream synchronisation followed by synchronize()) before the output is read.
    void processBlockDevice(const float *const *dIn, float *const *dOut, void *const *hipStreams = nullptr)
    {
        run([&](int g, Shard &sh) { sh.proc.processBlockDevice(dIn[g], dOut[g], hipStreams ? hipStreams[g] : nullptr); });
    }
    void processBlockMonoDevice(const float *const *dVoice, float *const *dOut, void *const *hipStreams = nullptr)   // voice [streams_g][N]
    {
        run([&](int g, Shard &sh) { sh.proc.processBlockMonoDevice(dVoice[g], dOut[g], hipStreams ? hipStreams[g] : nullptr); });
    }
    // nBlocks queued blocks per call: dIn[g] = [nBlocks][streams_g][3][N] -> dOut[g] = [nBlocks][streams_g][2][N] (reserveBlocks first)
    void processBlocksDevice(const float *const *dIn, float *const *dOut, int nBlocks, void *const *hipStreams = nullptr)
    {
        run([&](int g, Shard &sh) { sh.proc.processBlocksDevice(dIn[g], dOut[g], nBlocks, hipStreams ? hipStreams[g] : nullptr); });
    }
    void processBlocksMonoDevice(const float *const *dVoice, float *const *dOut, int nBlocks, void *const *hipStreams = nullptr)
    {
        run([&](int g, Shard &sh) { sh.proc.processBlocksMonoDevice(dVoice[g], dOut[g], nBlocks, hipStreams ? hipStreams[g] : nullptr); });
    }
    void reserveBlocks(int nBlocks) { run([&](int, Shard &sh) { sh.proc.reserveBlocks(nBlocks); }); }
    // every shard's device idle, and every shard's verdict (the first error is rethrown: VP_ERR_TIMEOUT / VP_ERR_HIP poison a handle)
    void synchronize() { run([&](int, Shard &sh) { sh.proc.synchronize(); }); }
    void setIirMode(int mode) { for (auto &sh : shards_) sh->proc.setIirMode(mode); }
    void setYinMode(int mode) { for (auto &sh : shards_) sh->proc.setYinMode(mode); }
    int device(int g) const { return shards_[g]->dev; }

private:
    struct Shard {
        BatchVocoderProcessor proc;
        int dev;
        std::thread worker;
        std::mutex m;
        std::condition_variable cv;
        std::function<void()> job;
        bool busy = false, quit = false;
        std::exception_ptr err;
        ~Shard()
        {
            { std::lock_guard<std::mutex> lk(m); quit = true; }
            cv.notify_all();
            if (worker.joinable()) worker.join();
        }
        explicit Shard(int dev_) : proc(dev_), dev(dev_)
        {
            worker = std::thread([this] {
                std::unique_lock<std::mutex> lk(m);
                for (;;) {
                    cv.wait(lk, [this] { return quit || busy; });
                    if (quit) return;
                    try { job(); } catch (...) { err = std::current_exception(); }
                    busy = false;
                    cv.notify_all();
                }
            });
        }
    };
    // fn(g, shard) on every shard's own thread, side by side; the first exception is rethrown here once all have finished
    template <class F>
    void run(F fn)
    {
        for (int g = 0; g < numShards(); g++) {
            Shard &sh = *shards_[g];
            { std::lock_guard<std::mutex> lk(sh.m); sh.job = [&fn, g, &sh] { fn(g, sh); }; sh.err = nullptr; sh.busy = true; }
            sh.cv.notify_all();
        }
        std::exception_ptr first;
        for (auto &shp : shards_) {
            std::unique_lock<std::mutex> lk(shp->m);
            shp->cv.wait(lk, [&] { return !shp->busy; });
            if (shp->err && !first) first = shp->err;
        }
        if (first) std::rethrow_exception(first);
    }
    std::pair<int, int> owner(int stream) const
    {
        if (stream < 0 || stream >= nStreams_) throw Error(VP_ERR_INVALID_ARG, "no such stream");
        for (int g = 0; g < numShards(); g++) {
            const auto r = shardRange(g);
            if (stream < r.first + r.second) return {g, stream - r.first};
        }
        return {numShards() - 1, 0};
    }
    std::vector<std::unique_ptr<Shard>> shards_;
    int nStreams_ = 0, N_ = 0;
};

// ------------------------------------------------------------------------------------------------
// vp::StreamingPitchTracker -- the streaming pitch tracker (vp_pv_tracker_*, vp_amd.h): one ratio per block and stream from the audio received
// so far (YIN on the last frameLen + ceil(sampleRate / 100) samples, the key's nearest note), the last voiced ratio held over holdBlocks
// unvoiced blocks, the ratio moved the fraction `glide` of the way to its target per block.  Its table is what
// StreamingPitchShifter::processBlocksCurve takes; StreamingPitchShifter::autotuneBlocks runs both.
class StreamingPitchTracker {
public:
    StreamingPitchTracker(int device, int nStreams, int blockSize, double sampleRate, int frameLen = 1024)
    {
        detail::check(vp_pv_tracker_create(device, nStreams, blockSize, frameLen, sampleRate, &t_), "vp_pv_tracker_create");
    }
    ~StreamingPitchTracker() { if (t_) vp_pv_tracker_destroy(t_); }
    StreamingPitchTracker(const StreamingPitchTracker &) = delete;
    StreamingPitchTracker &operator=(const StreamingPitchTracker &) = delete;

    // every stream, from the next process call on; 0 <= holdBlocks <= 2^20, 0 < glide <= 1 (defaults 0 and 1: the raw ratio)
    void setFollow(int holdBlocks, double glide) { detail::check(vp_pv_tracker_set_follow(t_, holdBlocks, glide), "setFollow"); }
    // takes effect at the next process call; stream = -1: all streams.  The shifter has its own reset.
    void reset(int stream = -1) { detail::check(vp_pv_tracker_reset(t_, stream), "reset"); }
    // device float [nBlocks][S][N] -> period int [nBlocks][S] and/or ratio double [nBlocks][S] (one may be null); dKey: device int [S] or
    // null (chromatic); enqueued on hipStream without synchronising
    void processBlocksDevice(const float *dIn, const int *dKey, int *dPeriod, double *dRatio, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_pv_tracker_process_blocks_device(t_, dIn, dKey, dPeriod, dRatio, nBlocks, hipStream), "processBlocksDevice");
    }
    // the key-aware voices (vp_pv_tracker_process_blocks_voices_device): dDegree device int [S][nVoices], steps of the key's table from the
    // note the tracker chose; dUnvoiced device double [S][nVoices] or null = 1; ratio double [nBlocks][S][nVoices], the table
    // StreamingHarmonizer::processBlocksDevice takes.  A block goes through this call or processBlocksDevice, not both
    void processBlocksVoices(const float *dIn, const int *dKey, int nVoices, const int *dDegree, const double *dUnvoiced, int *dPeriod,
                             double *dRatio, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_pv_tracker_process_blocks_voices_device(t_, dIn, dKey, nVoices, dDegree, dUnvoiced, dPeriod, dRatio, nBlocks, hipStream),
                      "processBlocksVoices");
    }
    // the fine tracker (VP_TRACK_FINE): the period refined below one sample, the note looked up on the refined pitch; from the next process
    // call on, for the mono call, the voices and the composed calls; touches no stream state
    void setFine(bool fine) { detail::check(vp_pv_tracker_set_mode(t_, fine ? VP_TRACK_FINE : VP_TRACK_INTEGER), "setFine"); }
    bool fine() const { return vp_pv_tracker_get_mode(t_) == VP_TRACK_FINE; }
    // processBlocksDevice with the fine tracker whatever the mode; dPeriodFine: device double [nBlocks][S] or null, the refined period of
    // the raw decision (0.0 on unvoiced blocks and while the ring fills)
    void processBlocksFine(const float *dIn, const int *dKey, int *dPeriod, double *dPeriodFine, double *dRatio, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_pv_tracker_process_blocks_fine_device(t_, dIn, dKey, dPeriod, dPeriodFine, dRatio, nBlocks, hipStream), "processBlocksFine");
    }
    vp_pv_tracker *handle() const { return t_; }

private:
    vp_pv_tracker *t_ = nullptr;
};

// vp::StreamingPitchShifter -- the streaming phase vocoder (vp_pv_*, vp_amd.h): S streams, blocks of N samples, state kept across calls.
// Output sample t of a stream is sample t - latency() of the one-shot vp_stft_pitch_shift on everything the stream received.
//
//     vp::StreamingPitchShifter ps(/*device*/ 0, /*streams*/ 256, /*block*/ 1024);   // hop 256
//     ps.setSemitones(7.0);                             // every stream; ps.setSemitones(-5.0, 3) for stream 3 alone
//     ps.processBlock(in, out);                         // float [256][1024] -> [256][1024], host memory, synchronous
class StreamingPitchShifter {
public:
    StreamingPitchShifter(int device, int nStreams, int blockSize, int hop = 256, int frameLen = 1024)
    {
        detail::check(vp_pv_create(device, nStreams, blockSize, frameLen, hop, &p_), "vp_pv_create");
    }
    ~StreamingPitchShifter() { if (p_) vp_pv_destroy(p_); }
    StreamingPitchShifter(const StreamingPitchShifter &) = delete;
    StreamingPitchShifter &operator=(const StreamingPitchShifter &) = delete;

    int latency() const { return vp_pv_get_latency(p_); }
    // takes effect at the next process call; stream = -1: all streams
    void setSemitones(double semitones, int stream = -1) { detail::check(vp_pv_set_semitones(p_, stream, semitones), "setSemitones"); }
    double semitones(int stream) const
    {
        double v = 0;
        detail::check(vp_pv_get_semitones(p_, stream, &v), "semitones");
        return v;
    }
    void reset(int stream = -1) { detail::check(vp_pv_reset(p_, stream), "reset"); }
    void processBlock(const float *in, float *out) { detail::check(vp_pv_process_block(p_, in, out), "processBlock"); }
    // device float [nBlocks][S][N], enqueued on hipStream without synchronising
    void processBlocksDevice(const float *dIn, float *dOut, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_pv_process_blocks_device(p_, dIn, dOut, nBlocks, hipStream), "processBlocksDevice");
    }
    // the same with one pitch RATIO per block and stream, device double [nBlocks][S] (vp_semitones_to_ratios converts intervals): a frame
    // takes the ratio of the block in which its last sample arrives; setSemitones' interval is neither used nor changed
    void processBlocksCurve(const float *dIn, float *dOut, const double *dRatio, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_pv_process_blocks_curve_device(p_, dIn, dOut, dRatio, nBlocks, hipStream), "processBlocksCurve");
    }
    // processBlocksCurve with peak locking (vp_pv_process_blocks_locked_device): a spectral peak's whole region of bins moves by one
    // integer offset and turns by one accumulated angle.  The kinds of call share the stream's state: after a change of kind the output
    // is finite but carries a phase jump -- reset() the stream at the change to avoid it
    void processBlocksLocked(const float *dIn, float *dOut, const double *dRatio, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_pv_process_blocks_locked_device(p_, dIn, dOut, dRatio, nBlocks, hipStream), "processBlocksLocked");
    }
    // processBlocksLocked with sub-bin region offsets (vp_pv_process_blocks_locked_subbin_device): a region is translated by the
    // real-valued offset of its peak's interpolated centre and the spectrum interpolated, so a shifted tone keeps its level
    void processBlocksLockedSubbin(const float *dIn, float *dOut, const double *dRatio, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_pv_process_blocks_locked_subbin_device(p_, dIn, dOut, dRatio, nBlocks, hipStream), "processBlocksLockedSubbin");
    }
    // automatic correction: the tracker's call, then processBlocksCurve along its table (dRatio: result and scratch, required; dPeriod
    // may be null), on one stream.  The tracker must have this shifter's streams, block size and device.  reset() does not reach it.
    void autotuneBlocks(StreamingPitchTracker &tracker, const float *dIn, float *dOut, const int *dKey, int *dPeriod, double *dRatio, int nBlocks,
                        void *hipStream = nullptr)
    {
        detail::check(vp_pv_autotune_blocks_device(p_, tracker.handle(), dIn, dOut, dKey, dPeriod, dRatio, nBlocks, hipStream), "autotuneBlocks");
    }
    // processBlocksCurve with the spectral envelope kept apart from the pitch (vp_pv_process_blocks_formant_device): dFormant device double
    // [S] of formant ratios, or null = 1.0 (the formants stay where they were); lifter: the cepstral lifter's length, 4 .. 64 samples.
    // The stream's state is the curve call's: formant, curve and plain calls mix freely
    void processBlocksFormant(const float *dIn, float *dOut, const double *dRatio, const double *dFormant, int nBlocks, int lifter = 32,
                              void *hipStream = nullptr)
    {
        detail::check(vp_pv_process_blocks_formant_device(p_, dIn, dOut, dRatio, dFormant, lifter, nBlocks, hipStream), "processBlocksFormant");
    }
    // automatic correction that keeps the formants: the tracker's call, then processBlocksFormant along its table
    void autotuneBlocks(StreamingPitchTracker &tracker, const float *dIn, float *dOut, const int *dKey, int *dPeriod, double *dRatio,
                        const double *dFormant, int lifter, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_pv_autotune_blocks_formant_device(p_, tracker.handle(), dIn, dOut, dKey, dPeriod, dRatio, dFormant, lifter, nBlocks,
                                                           hipStream),
                      "autotuneBlocks (formant)");
    }
    vp_pv *handle() const { return p_; }

private:
    vp_pv *p_ = nullptr;
};

// vp::StreamingCrossSynth -- the streaming STFT cross-synthesis (vp_xs_*, vp_amd.h): S pairs of voice and carrier, blocks of N samples,
// state kept across calls.  Output sample t of a stream is sample t - latency() of the one-shot vp_stft_cross_synth on everything the
// stream received: the carrier with the voice's spectral envelope.
//
//     vp::StreamingCrossSynth xs(/*device*/ 0, /*streams*/ 256, /*block*/ 1024);     // hop 256
//     xs.processBlocksDevice(dVoice, dCarrier, dOut, /*dDepth*/ nullptr, 16);        // device float [16][256][1024] each
class StreamingCrossSynth {
public:
    StreamingCrossSynth(int device, int nStreams, int blockSize, int hop = 256, int frameLen = 1024)
    {
        detail::check(vp_xs_create(device, nStreams, blockSize, frameLen, hop, &x_), "vp_xs_create");
    }
    ~StreamingCrossSynth() { if (x_) vp_xs_destroy(x_); }
    StreamingCrossSynth(const StreamingCrossSynth &) = delete;
    StreamingCrossSynth &operator=(const StreamingCrossSynth &) = delete;

    int latency() const { return vp_xs_get_latency(x_); }
    // takes effect at the next process call; stream = -1: all streams
    void reset(int stream = -1) { detail::check(vp_xs_reset(x_, stream), "reset"); }
    // device float [nBlocks][S][N] each, dOut no alias of an input; dDepth: device double [S] in [0, 1] or null = 1 (0: the carrier's
    // plain round trip); lifter: the cepstral lifter's length, 4 .. 64 samples; enqueued on hipStream without synchronising
    void processBlocksDevice(const float *dVoice, const float *dCarrier, float *dOut, const double *dDepth, int nBlocks, int lifter = 32,
                             void *hipStream = nullptr)
    {
        detail::check(vp_xs_process_blocks_device(x_, dVoice, dCarrier, dOut, dDepth, lifter, nBlocks, hipStream), "processBlocksDevice");
    }
    long debugAllocCount() const { return vp_xs_debug_alloc_count(x_); }
    vp_xs *handle() const { return x_; }

private:
    vp_xs *x_ = nullptr;
};

// vp::StreamingHarmonizer -- the streaming phase-vocoder harmonizer (vp_hz_*, vp_amd.h): S streams, blocks of N samples, nVoices
// peak-locked voices per stream beside the dry signal, state kept across calls.  Output sample t of a stream is sample t - latency() of
// the one-shot vp_stft_harmonize on everything the stream received; the dry part is delayed with the voices.
//
//     vp::StreamingHarmonizer hz(/*device*/ 0, /*streams*/ 256, /*block*/ 1024, /*voices*/ 3);      // hop 256
//     hz.processBlocksDevice(dIn, dOut, dRatio, /*dGain*/ nullptr, dDry, 16);   // float [16][256][1024]; double [16][256][3], -, [256]
class StreamingHarmonizer {
public:
    StreamingHarmonizer(int device, int nStreams, int blockSize, int nVoices, int hop = 256, int frameLen = 1024)
    {
        detail::check(vp_hz_create(device, nStreams, blockSize, frameLen, hop, nVoices, &h_), "vp_hz_create");
    }
    ~StreamingHarmonizer() { if (h_) vp_hz_destroy(h_); }
    StreamingHarmonizer(const StreamingHarmonizer &) = delete;
    StreamingHarmonizer &operator=(const StreamingHarmonizer &) = delete;

    int latency() const { return vp_hz_get_latency(h_); }
    // takes effect at the next process call; stream = -1: all streams
    void reset(int stream = -1) { detail::check(vp_hz_reset(h_, stream), "reset"); }
    // dIn, dOut: device float [nBlocks][S][N]; dRatio: device double [nBlocks][S][nVoices], pitch ratios in [0.5, 2]; dGain: device double
    // [S][nVoices] or null = 1; dDry: device double [S] or null = 0; enqueued on hipStream without synchronising
    void processBlocksDevice(const float *dIn, float *dOut, const double *dRatio, const double *dGain, const double *dDry, int nBlocks,
                             void *hipStream = nullptr)
    {
        detail::check(vp_hz_process_blocks_device(h_, dIn, dOut, dRatio, dGain, dDry, nBlocks, hipStream), "processBlocksDevice");
    }
    // tracker.processBlocksVoices with this handle's voice count, then processBlocksDevice along its table, on the same stream
    // (vp_hz_autoharm_blocks_device): dRatio [nBlocks][S][nVoices] is result and scratch, dPeriod may be null.  Resets stay separate
    void autoharmBlocks(StreamingPitchTracker &tracker, const float *dIn, float *dOut, const int *dKey, const int *dDegree, const double *dUnvoiced,
                        const double *dGain, const double *dDry, int *dPeriod, double *dRatio, int nBlocks, void *hipStream = nullptr)
    {
        detail::check(vp_hz_autoharm_blocks_device(h_, tracker.handle(), dIn, dOut, dKey, dDegree, dUnvoiced, dGain, dDry, dPeriod, dRatio, nBlocks,
                                                   hipStream), "autoharmBlocks");
    }
    long debugAllocCount() const { return vp_hz_debug_alloc_count(h_); }
    vp_hz *handle() const { return h_; }

private:
    vp_hz *h_ = nullptr;
};

}  // namespace vp
