// Header-only C++ host adaptor over the C ABI's ADPCM audio encoder (include/fmdemod.h "ADPCM audio encoder"): RAII around the handle,
// the device arrays it writes and one WAV file per station (format tag 0x0011, IMA / DVI ADPCM, which ordinary players open),
// exceptions instead of status codes.  NOT in the reference (williamyang98/FM-Radio's scraper writes 16-bit PCM, four times the
// bytes: fm_scraper_writer.hpp); it reads the station audio [C][in_stride][2] f32 that the mixer and the monitors read:
//
//   fmd_host::AdpcmRecorder_GPU rec(paths, 32000, frames_per_block);     // one path per station; every file stays open
//   rec.Process(d_audio, in_stride, n, d_active, stream);                // encodes, waits, appends each station's completed blocks
//   rec.Close();                                                         // (or the destructor) flushes the open blocks, rewrites the headers
//
// A file is valid after every Process: its header is rewritten with the blocks so far.  After Close its `fact` chunk states the frames
// the station was fed, without the flush's padding.  The process's open-file limit has to cover the stations.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "fmdemod.h"

namespace fmd_host {

class AdpcmRecorder_GPU {
    fmd_adpcm e = nullptr;
    int n_channels, fs, block_frames, block_align;
    long long max_blocks;                    // of one Process call
    uint8_t* d_out = nullptr;                // [C][max_blocks * block_align]
    int* d_nblocks = nullptr;                // [C]
    std::vector<uint8_t> out;
    std::vector<int> nblocks;
    std::vector<FILE*> files;
    std::vector<long long> written;          // blocks in each file
    std::vector<fmd_adpcm_status> status;
    bool closed = false;
    void check(int rc, const char* what) const { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + fmd_adpcm_last_error(e)); }
    void header(int c, long long frames) {
        uint8_t h[FMD_ADPCM_WAV_HEADER_BYTES];
        int len = 0;
        if (fmd_adpcm_wav_header(fs, block_frames, written[(size_t)c], frames, h, &len) != FMD_OK) throw std::runtime_error(std::string("fmd_adpcm_wav_header: ") + fmd_adpcm_last_error(nullptr));
        FILE* fp = files[(size_t)c];
        if (fseek(fp, 0, SEEK_SET) != 0 || fwrite(h, 1, (size_t)len, fp) != (size_t)len || fseek(fp, 0, SEEK_END) != 0) throw std::runtime_error("AdpcmRecorder_GPU: a header's write failed");
    }
    // the counts and the completed blocks to the host, behind the work on `stream`, and into the files; headers state whole blocks
    void collect(long long rows_blocks, void* stream) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (hipMemcpyAsync(nblocks.data(), d_nblocks, sizeof(int) * (size_t)n_channels, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            throw std::runtime_error("AdpcmRecorder_GPU: the counts' copy failed");
        long long most = 0;
        for (int c = 0; c < n_channels; c++) most = nblocks[(size_t)c] > most ? nblocks[(size_t)c] : most;
        if (most == 0) return;
        if (most > rows_blocks) throw std::runtime_error("AdpcmRecorder_GPU: more blocks than the call can complete");
        const size_t pitch = (size_t)(max_blocks * block_align), width = (size_t)(most * block_align);
        if (hipMemcpy2D(out.data(), pitch, d_out, pitch, width, (size_t)n_channels, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("AdpcmRecorder_GPU: the blocks' copy failed");
        for (int c = 0; c < n_channels; c++) {
            const size_t bytes = (size_t)nblocks[(size_t)c] * (size_t)block_align;
            if (bytes == 0) continue;
            if (fwrite(out.data() + (size_t)c * pitch, 1, bytes, files[(size_t)c]) != bytes) throw std::runtime_error("AdpcmRecorder_GPU: a file's write failed");
            written[(size_t)c] += nblocks[(size_t)c];
            header(c, written[(size_t)c] * block_frames);
        }
    }
    void release() {
        for (FILE* fp : files) if (fp) fclose(fp);
        files.clear();
        if (e) fmd_adpcm_destroy(e);
        e = nullptr;
        if (d_out) (void)hipFree(d_out);
        if (d_nblocks) (void)hipFree(d_nblocks);
        d_out = nullptr; d_nblocks = nullptr;
    }
public:
    // block_frames: 0 = 1017 (1024-byte blocks)
    AdpcmRecorder_GPU(const std::vector<std::string>& paths, int _fs, long long max_input_frames, int _block_frames = 0, int device = -1)
        : n_channels((int)paths.size()), fs(_fs), block_frames(_block_frames), block_align(0), max_blocks(0) {
        fmd_adpcm_config cfg{n_channels, _block_frames, max_input_frames, device};
        if (fmd_adpcm_create(&cfg, &e) != FMD_OK) throw std::runtime_error(std::string("fmd_adpcm_create: ") + fmd_adpcm_last_error(nullptr));
        block_align = fmd_adpcm_block_align(_block_frames);
        block_frames = (block_align / 8 - 1) * 8 + 1;
        max_blocks = fmd_adpcm_max_blocks(block_frames, max_input_frames);
        if (max_blocks < 1) max_blocks = 1;                                  // (the flush's block)
        const size_t C = (size_t)n_channels;
        out.resize(C * (size_t)(max_blocks * block_align));
        nblocks.assign(C, 0); written.assign(C, 0); status.resize(C); files.assign(C, nullptr);
        try {
            // (create has made `device` current where one was given)
            if (hipMalloc(reinterpret_cast<void**>(&d_out), out.size()) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d_nblocks), sizeof(int) * C) != hipSuccess ||
                hipMemset(d_nblocks, 0, sizeof(int) * C) != hipSuccess)
                throw std::runtime_error("AdpcmRecorder_GPU: the outputs' allocation failed");
            for (size_t c = 0; c < C; c++) {
                files[c] = fopen(paths[c].c_str(), "wb+");
                if (!files[c]) throw std::runtime_error("AdpcmRecorder_GPU: cannot open " + paths[c]);
                header((int)c, 0);
            }
        } catch (...) {
            release();
            throw;
        }
    }
    ~AdpcmRecorder_GPU() {
        try { Close(); } catch (...) {}
        release();
    }
    AdpcmRecorder_GPU(const AdpcmRecorder_GPU&) = delete;
    AdpcmRecorder_GPU& operator=(const AdpcmRecorder_GPU&) = delete;

    int GetTotalChannels() const { return n_channels; }
    int GetBlockFrames() const { return block_frames; }
    int GetBlockAlign() const { return block_align; }
    long long BlocksWritten(int c) const { return written.at((size_t)c); }

    // takes n frames of every station whose d_active byte is not 0 (NULL: all), waits for the work on `stream` and appends each
    // station's completed blocks to its file
    void Process(const float* d_in, long long in_stride, long long n, const uint8_t* d_active = nullptr, void* stream = nullptr) {
        if (closed) throw std::runtime_error("AdpcmRecorder_GPU: closed");
        check(fmd_adpcm_process_f32_dev(e, d_in, in_stride, n, d_active, d_out, max_blocks * block_align, d_nblocks, stream), "fmd_adpcm_process_f32_dev");
        collect(max_blocks, stream);
    }
    // closes every station's open block with repeats of its last frame, appends it, and rewrites every header with the frames the
    // station was fed; the files are complete afterwards.  Safe to repeat
    void Close(void* stream = nullptr) {
        if (closed || !e) return;
        closed = true;
        check(fmd_adpcm_flush(e, -1, d_out, max_blocks * block_align, d_nblocks, stream), "fmd_adpcm_flush");
        collect(1, stream);
        check(fmd_adpcm_get_status(e, status.data()), "fmd_adpcm_get_status");
        for (int c = 0; c < n_channels; c++) {
            header(c, (long long)status[(size_t)c].frames);
            fflush(files[(size_t)c]);
        }
    }
    // waits for the encoder's work and copies every station's record to the host
    void Update() { check(fmd_adpcm_get_status(e, status.data()), "fmd_adpcm_get_status"); }
    // as of the last Update() or Close()
    const fmd_adpcm_status& Status(int c) const { return status.at((size_t)c); }
    // the device's own records, for a consumer on the device (valid until the next Process)
    const fmd_adpcm_status* StatusDev() const {
        const fmd_adpcm_status* p = nullptr;
        check(fmd_adpcm_status_dev(e, &p), "fmd_adpcm_status_dev");
        return p;
    }
};

}  // namespace fmd_host
