// Test driver: the reference app's listener path (src/fm_demod_tuner.cpp:145-165 -> AudioMixer::UpdateMixer, src/audio/
// portaudio_output.cpp:84) with the demodulator and the mixer on the GPU.  Bus 0 plays every station of the capture, bus 1 station 0
// alone at gain 2.5 (clipping); bus 0's frames go to a WAV file, block after block.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "audio_mixer_gpu.hpp"
#include "fm_scraper_writer.hpp"

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: mixer_main <capture.cf32 [C][n][2]> <n_channels> <block_size> <fs_baseband> <out.wav>\n"); return 1; }
    const int C = atoi(argv[2]), bs = atoi(argv[3]), fs = atoi(argv[4]);
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
    fmd_host::AudioMixer_GPU mixer(C, 2);
    for (int c = 0; c < C; c++) mixer.AddSource(0, c);
    mixer.AddSource(1, 0);
    mixer.GetOutputGain(1) = 2.5f;
    fmd_host::Audio_WAV_Writer wav(argv[5], rates.fs_audio);
    std::vector<float> block((size_t)C * bs * 2);
    long long total = 0;
    for (size_t b = 0; b < n_blocks; b++) {
        for (int c = 0; c < C; c++)
            for (size_t i = 0; i < (size_t)bs * 2; i++) block[(size_t)c * bs * 2 + i] = cap[((size_t)c * n + b * bs) * 2 + i];
        if (fmd_process_cf32_host(h, block.data(), C, bs) != FMD_OK) { fprintf(stderr, "fmd_process: %s\n", fmd_last_error(h)); return 4; }
        const float* d_audio = nullptr;
        fmd_audio_dev(h, &d_audio);
        total += mixer.UpdateMixer(d_audio, rates.n_audio, rates.n_audio);
        wav.on_audio_data(mixer.Bus(0), (size_t)mixer.GetFrames());
    }
    fmd_destroy(h);
    printf("%zu blocks, %lld frames per bus at %d Hz\n", n_blocks, total, rates.fs_audio);
    return 0;
}
