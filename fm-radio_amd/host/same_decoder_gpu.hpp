// Header-only C++ host adaptor over the C ABI's EAS SAME decoder (include/fmdemod.h "EAS SAME decoder"): RAII around the handle and the
// two device byte arrays it writes, exceptions instead of status codes, and the messages accepted since they were last asked for.  NOT
// in the reference (williamyang98/FM-Radio plays one station to a listener): it reads the station audio [C][in_stride][2] f32 that the
// mixer and the monitors read, and its flags are a recorder's or a mixer bus's trigger:
//
//   fmd_host::SameDecoder_GPU dec(n_channels, 32000, frames_per_block);
//   dec.Process(d_audio, in_stride, n, nullptr, stream);               // asynchronous on the stream given
//   mixer.Process(..., dec.FlagsDev(), stream);                        // FMD_SAME_ALERT_OPEN != 0: an alert bus of the stations in alert
//   dec.Update();                                                      // waits, reads 2856 bytes and the two bytes per station
//   for (const fmd_same_message& m : dec.NewMessages(c)) { fmd_same_header h; fmd_same_parse(m.bytes, m.len, &h); ... }
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class SameDecoder_GPU {
    fmd_same d = nullptr;
    int n_channels, fs;
    uint8_t* d_bytes = nullptr;              // [2][C]: flags, ok
    std::vector<fmd_same_status> status;
    std::vector<unsigned long long> seen;    // per station: the accepted messages handed out
    std::vector<uint8_t> bytes;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_same_last_error(d)); }
public:
    SameDecoder_GPU(int _n_channels, int _fs, long long max_input_frames, int device = -1)
        : n_channels(_n_channels), fs(_fs), status((size_t)(_n_channels > 0 ? _n_channels : 0)), seen(status.size(), 0ull), bytes(2 * status.size()) {
        fmd_same_config cfg{_n_channels, _fs, max_input_frames, device};
        if (fmd_same_create(&cfg, &d) != FMD_OK) throw std::runtime_error(std::string("fmd_same_create: ") + fmd_same_last_error(nullptr));
        // (create has made `device` current where one was given); before the first Process every flag is clear and every station ok
        if (hipMalloc(reinterpret_cast<void**>(&d_bytes), bytes.size()) != hipSuccess || hipMemset(d_bytes, 0, status.size()) != hipSuccess ||
            hipMemset(d_bytes + status.size(), 1, status.size()) != hipSuccess) {
            fmd_same_destroy(d);
            throw std::runtime_error("SameDecoder_GPU: the bytes' allocation failed");
        }
    }
    ~SameDecoder_GPU() {
        if (d) fmd_same_destroy(d);
        if (d_bytes) (void)hipFree(d_bytes);
    }
    SameDecoder_GPU(const SameDecoder_GPU&) = delete;
    SameDecoder_GPU& operator=(const SameDecoder_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    int GetSampleRate() const { return fs; }
    // the [C] uint8 arrays on the device, written behind every Process on its stream; either is another object's d_active
    const uint8_t* FlagsDev() const { return d_bytes; }
    const uint8_t* OkDev() const { return d_bytes + status.size(); }

    // takes n frames of every station whose d_active byte is not 0 (NULL: all) and writes their two bytes; asynchronous on `stream`
    void Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        check(fmd_same_process_f32_dev(d, d_in, in_stride, n, d_active, d_bytes, d_bytes + status.size(), stream), "fmd_same_process_f32_dev");
    }
    void Reset(int channel = -1) {
        check(fmd_same_reset(d, channel), "fmd_same_reset");
        for (size_t c = 0; c < seen.size(); c++)
            if (channel < 0 || (size_t)channel == c) seen[c] = 0ull;
    }
    void SetParams(const fmd_same_params& p, int channel = -1) { check(fmd_same_set_params(d, channel, &p), "fmd_same_set_params"); }
    fmd_same_params GetParams(int channel) const {
        fmd_same_params p;
        check(fmd_same_get_params(d, channel, &p), "fmd_same_get_params");
        return p;
    }

    // waits for the decoder's work and copies every station's record and two bytes to the host
    void Update() {
        check(fmd_same_get_status(d, status.data()), "fmd_same_get_status");
        if (hipMemcpy(bytes.data(), d_bytes, bytes.size(), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("SameDecoder_GPU: the bytes' copy failed");
    }
    // as of the last Update()
    const fmd_same_status& Status(int c) const { return status.at((size_t)c); }
    unsigned Flags(int c) const { return bytes.at((size_t)c); }
    bool IsOk(int c) const { return bytes.at(status.size() + (size_t)c) != 0; }
    bool AlertOpen(int c) const { return (Flags(c) & FMD_SAME_ALERT_OPEN) != 0; }
    // station c's messages accepted since the last NewMessages(c), oldest first (of more than eight the newest eight)
    std::vector<fmd_same_message> NewMessages(int c) {
        const fmd_same_status& s = Status(c);
        unsigned long long k = seen.at((size_t)c);
        if (s.accepted > FMD_SAME_RING && k < s.accepted - FMD_SAME_RING) k = s.accepted - FMD_SAME_RING;
        std::vector<fmd_same_message> out;
        for (; k < s.accepted; k++) out.push_back(s.ring[k % FMD_SAME_RING]);
        seen[(size_t)c] = s.accepted;
        return out;
    }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_same_status* StatusDev() const {
        const fmd_same_status* p = nullptr;
        check(fmd_same_status_dev(d, &p), "fmd_same_status_dev");
        return p;
    }
};

}  // namespace fmd_host
