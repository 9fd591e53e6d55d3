// Test driver: the reference tuner's audio path (src/fm_demod_tuner.cpp:145-165: OnAudioBlock -> SetInputSampleRate ->
// ConsumeBuffer) with the demodulator and the player on the GPU, channel 0's resampled audio written to a WAV file at the output rate.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fm_scraper_writer.hpp"
#include "resampled_pcm_player_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: resample_player_main <capture.cf32 [C][n][2]> <n_channels> <block_size> <fs_baseband> <fs_out> <out.wav>\n"); return 1; }
    const int C = atoi(argv[2]), bs = atoi(argv[3]), fs = atoi(argv[4]), fs_out = atoi(argv[5]);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    fseek(fp, 0, SEEK_END); const long bytes = ftell(fp); fseek(fp, 0, SEEK_SET);
    std::vector<float> cap((size_t)bytes / 4);
    if (fread(cap.data(), 4, cap.size(), fp) != cap.size()) return 2;
    fclose(fp);
    const size_t n = cap.size() / 2 / (size_t)C, n_blocks = n / (size_t)bs;
    fmd_config cfg{C, bs, fs, -1, 0u};
    fmd_handle h = nullptr;
    if (fmd_create(&cfg, &h) != FMD_OK) { fprintf(stderr, "fmd_create: %s\n", fmd_last_error(nullptr)); return 3; }
    fmd_rates rates{};
    fmd_get_rates(h, &rates);
    fmd_host::Resampled_PCM_Player_GPU player(C, fs_out, FMD_RESAMPLE_POLYPHASE, rates.n_audio);
    fmd_host::Audio_WAV_Writer wav(argv[6], player.GetOutputSampleRate());
    player.OnAudioOut([&](int c, const float* frames, size_t n_frames, int) { if (c == 0) wav.on_audio_data(frames, n_frames); });
    std::vector<float> block((size_t)C * bs * 2);
    long long total = 0;
    for (size_t b = 0; b < n_blocks; b++) {
        for (int c = 0; c < C; c++)
            for (size_t i = 0; i < (size_t)bs * 2; i++) block[(size_t)c * bs * 2 + i] = cap[((size_t)c * n + b * bs) * 2 + i];
        if (fmd_process_cf32_host(h, block.data(), C, bs) != FMD_OK) { fprintf(stderr, "fmd_process: %s\n", fmd_last_error(h)); return 4; }
        const float* d_audio = nullptr;
        fmd_audio_dev(h, &d_audio);
        player.SetInputSampleRate(rates.fs_audio);
        total += player.ConsumeBuffer(d_audio, rates.n_audio, rates.n_audio);
    }
    fmd_destroy(h);
    printf("%zu blocks, %lld frames at %d Hz\n", n_blocks, total, fs_out);
    return 0;
}
