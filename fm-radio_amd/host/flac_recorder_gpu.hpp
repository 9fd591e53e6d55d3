// Header-only C++ host adaptor over the C ABI's FLAC audio encoder (include/fmdemod.h "FLAC audio encoder"): RAII around the handle,
// the device arrays it writes and one .flac file per station and stream, exceptions instead of status codes.  NOT in the reference
// (williamyang98/FM-Radio's scraper writes 16-bit PCM: fm_scraper_writer.hpp); it reads the station audio [C][in_stride][2] f32 that the
// mixer and the monitors read, and its files decode to exactly the PCM fmd_audio_pcm16_dev writes:
//
//   fmd_host::FlacRecorder_GPU rec(stems, 32000, frames_per_block);      // one path stem per station: <stem>_<stream>.flac
//   rec.Process(d_audio, in_stride, n, d_active, stream);                // encodes, waits, appends each station's completed FLAC frames
//   rec.EndStream(c);                                                    // a short last frame, STREAMINFO rewritten, the next stream's file opens with its first frame
//   rec.Close();                                                         // (or the destructor) ends every stream
//
// A file can be played after every Process: its STREAMINFO then says "unknown" (zeros) for the length and the frame sizes, which the
// format allows.  After EndStream or Close it states the stream's samples and its smallest and largest frame, from the station's
// record; the MD5 signature stays zero ("not computed").  A stream that ends by itself because its frame number would reach 2^31
// (fmd_flac_status.wrapped; 33 days at S = 64 and 48 kHz, 8.7 years at the default and 32 kHz) is not split into a file of its own.  The process's
// open-file limit has to cover the stations.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class FlacRecorder_GPU {
    fmd_flac e = nullptr;
    int n_channels, fs, block_frames;
    long long pitch;                         // bytes of a station's row of d_out: what one Process call may write
    uint8_t* d_out = nullptr;                // [C][pitch]
    int* d_nbytes = nullptr;                 // [C]
    std::vector<uint8_t> out;
    std::vector<int> nbytes;
    std::vector<std::string> stems;
    std::vector<FILE*> files;                // the current stream's file, or null until the stream's first frame
    std::vector<unsigned> stream_index;      // of the current stream, per station
    std::vector<long long> file_bytes;       // FLAC frame bytes in the current file
    std::vector<fmd_flac_status> status;
    bool closed = false;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_flac_last_error(e)); }
    void header(int c, long long samples, unsigned minb, unsigned maxb) {
        uint8_t h[FMD_FLAC_STREAM_HEADER_BYTES];
        int len = 0;
        if (fmd_flac_stream_header(fs, block_frames, samples, (int)minb, (int)maxb, h, &len) != FMD_OK)
            throw std::runtime_error(std::string("fmd_flac_stream_header: ") + fmd_flac_last_error(nullptr));
        FILE* fp = files[(size_t)c];
        if (fseek(fp, 0, SEEK_SET) != 0 || fwrite(h, 1, (size_t)len, fp) != (size_t)len || fseek(fp, 0, SEEK_END) != 0) throw std::runtime_error("FlacRecorder_GPU: a header's write failed");
    }
    void open(int c) {
        const std::string path = stems[(size_t)c] + "_" + std::to_string(stream_index[(size_t)c]) + ".flac";
        files[(size_t)c] = fopen(path.c_str(), "wb+");
        if (!files[(size_t)c]) throw std::runtime_error("FlacRecorder_GPU: cannot open " + path);
        file_bytes[(size_t)c] = 0;
        header(c, 0, 0, 0);
    }
    // the counts and the frames to the host, behind the work on `stream`, and into the files
    void collect(int c0, int cn, void* stream) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (hipMemcpyAsync(nbytes.data() + c0, d_nbytes + c0, sizeof(int) * (size_t)cn, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            throw std::runtime_error("FlacRecorder_GPU: the counts' copy failed");
        long long most = 0;
        for (int c = c0; c < c0 + cn; c++) most = nbytes[(size_t)c] > most ? nbytes[(size_t)c] : most;
        if (most == 0) return;
        if (most > pitch) throw std::runtime_error("FlacRecorder_GPU: more bytes than the call can write");
        if (hipMemcpy2D(out.data() + (size_t)c0 * (size_t)pitch, (size_t)pitch, d_out + (size_t)c0 * (size_t)pitch, (size_t)pitch, (size_t)most, (size_t)cn, hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("FlacRecorder_GPU: the frames' copy failed");
        for (int c = c0; c < c0 + cn; c++) {
            const size_t bytes = (size_t)nbytes[(size_t)c];
            if (bytes == 0) continue;
            if (!files[(size_t)c]) open(c);
            if (fwrite(out.data() + (size_t)c * (size_t)pitch, 1, bytes, files[(size_t)c]) != bytes) throw std::runtime_error("FlacRecorder_GPU: a file's write failed");
            file_bytes[(size_t)c] += (long long)bytes;
        }
    }
    void release() {
        for (FILE* fp : files) if (fp) fclose(fp);
        files.clear();
        if (e) fmd_flac_destroy(e);
        e = nullptr;
        if (d_out) (void)hipFree(d_out);
        if (d_nbytes) (void)hipFree(d_nbytes);
        d_out = nullptr; d_nbytes = nullptr;
    }
public:
    // block_frames: 0 = 4096
    FlacRecorder_GPU(const std::vector<std::string>& _stems, int _fs, long long max_input_frames, int _block_frames = 0, int device = -1)
        : n_channels((int)_stems.size()), fs(_fs), block_frames(_block_frames), pitch(0), stems(_stems) {
        fmd_flac_config cfg{n_channels, _block_frames, _fs, max_input_frames, device};
        if (fmd_flac_create(&cfg, &e) != FMD_OK) throw std::runtime_error(std::string("fmd_flac_create: ") + fmd_flac_last_error(nullptr));
        block_frames = _block_frames == 0 ? 4096 : _block_frames;
        pitch = fmd_flac_max_bytes(block_frames, max_input_frames);
        const long long one = fmd_flac_max_bytes(block_frames, 1);          // (the flush's frame)
        if (pitch < one) pitch = one;
        const size_t C = (size_t)n_channels;
        out.resize(C * (size_t)pitch);
        nbytes.assign(C, 0); stream_index.assign(C, 0u); file_bytes.assign(C, 0); status.resize(C); files.assign(C, nullptr);
        try {
            // (create has made `device` current where one was given)
            if (hipMalloc(reinterpret_cast<void**>(&d_out), out.size()) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d_nbytes), sizeof(int) * C) != hipSuccess ||
                hipMemset(d_nbytes, 0, sizeof(int) * C) != hipSuccess)
                throw std::runtime_error("FlacRecorder_GPU: the outputs' allocation failed");
            for (size_t c = 0; c < C; c++) open((int)c);
        } catch (...) {
            release();
            throw;
        }
    }
    ~FlacRecorder_GPU() {
        try { Close(); } catch (...) {}
        release();
    }
    FlacRecorder_GPU(const FlacRecorder_GPU&) = delete;
    FlacRecorder_GPU& operator=(const FlacRecorder_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    int GetBlockFrames() const { return block_frames; }
    unsigned StreamIndex(int c) const { return stream_index.at((size_t)c); }
    long long FileBytes(int c) const { return file_bytes.at((size_t)c); }

    // takes n frames of every station whose d_active byte is not 0 (NULL: all), waits for the work on `stream` and appends each
    // station's completed FLAC frames to its file
    void Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        if (closed) throw std::runtime_error("FlacRecorder_GPU: closed");
        check(fmd_flac_process_f32_dev(e, d_in, in_stride, n, d_active, d_out, pitch, d_nbytes, nullptr, stream), "fmd_flac_process_f32_dev");
        collect(0, n_channels, stream);
    }
    // ends the stream of station c (-1: of every station): the open block leaves as a short last frame, the file's STREAMINFO is
    // rewritten from the station's record and the file closed; the next stream's file opens with its first frame
    void EndStream(int c = -1, void* stream = nullptr) {
        if (closed) throw std::runtime_error("FlacRecorder_GPU: closed");
        if (c < -1 || c >= n_channels) throw std::runtime_error("FlacRecorder_GPU: no such station");
        const int c0 = c < 0 ? 0 : c, cn = c < 0 ? n_channels : 1;
        check(fmd_flac_get_status(e, status.data()), "fmd_flac_get_status");                  // the stream's counters, before the flush clears them
        check(fmd_flac_flush(e, c, d_out, pitch, d_nbytes, nullptr, stream), "fmd_flac_flush");
        collect(c0, cn, stream);
        for (int i = c0; i < c0 + cn; i++) {
            const fmd_flac_status& st = status[(size_t)i];
            const unsigned last = (unsigned)nbytes[(size_t)i];
            unsigned minb = st.min_frame_bytes, maxb = st.max_frame_bytes;
            if (last > 0) { minb = minb == 0 || last < minb ? last : minb; maxb = last > maxb ? last : maxb; }
            if (files[(size_t)i]) {
                header(i, (long long)(st.stream_samples + st.fill), minb, maxb);
                if (fclose(files[(size_t)i]) != 0) { files[(size_t)i] = nullptr; throw std::runtime_error("FlacRecorder_GPU: a file's close failed"); }
                files[(size_t)i] = nullptr;
            }
            stream_index[(size_t)i]++;
        }
        check(fmd_flac_get_status(e, status.data()), "fmd_flac_get_status");
    }
    // ends every stream; the files are complete afterwards.  Safe to repeat
    void Close(void* stream = nullptr) {
        if (closed || !e) return;
        EndStream(-1, stream);
        closed = true;
    }
    // waits for the encoder's work and copies every station's record to the host
    void Update() { check(fmd_flac_get_status(e, status.data()), "fmd_flac_get_status"); }
    // as of the last Update(), EndStream() or Close()
    const fmd_flac_status& Status(int c) const { return status.at((size_t)c); }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_flac_status* StatusDev() const {
        const fmd_flac_status* p = nullptr;
        check(fmd_flac_status_dev(e, &p), "fmd_flac_status_dev");
        return p;
    }
};

}  // namespace fmd_host
