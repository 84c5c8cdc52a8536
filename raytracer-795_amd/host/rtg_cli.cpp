// rtg_cli — the reference's command line (`./raytracer scene.xml`, src/main.cpp:7-14) on the
// MI355X path: parse the scene (rtgh_parse_xml), build it on the GPU, render and save every
// camera (rtgh_render_scene).
//
//   rtg_cli scene.xml [--device N] [--devices G] [--seed S] [--out-dir DIR]
//
// --devices G renders every camera on G GPUs (device N and the next G-1): one host thread per
// GPU, row-block pixel shards, RCCL gather of the rows onto device N -- the reference's
// renderScene fork over 8 std::threads (src/Scene.cpp:294-363, threads at 340-356) moved to GPUs.
//
//   rtg_cli scene.xml --progressive K [--target-error E] [--device N] [--seed S] [--out-dir DIR]
//
// --progressive K renders every camera in rounds of K samples on a resumable frame (rtg_frame): after each
// round the image files are rewritten and a line with the samples done, the mean standard error of the
// pixels' luminance and their mean luminance is printed.  --target-error E stops a camera after the first
// round with mean_sem <= E x mean_luminance; without it (or with E = 0) the render runs to NumSamples and
// the files equal those of a run without --progressive, byte for byte.  One GPU only.
//
//   rtg_cli scene.xml --progressive K --adaptive REL [--min-samples M] ...
//
// --adaptive REL (with --progressive) samples adaptively: after each round the pixels whose standard error is
// at most REL x their mean luminance (and that hold at least M samples, default 2) are retired and traced no
// further; the round's line also reports the active pixels, and a camera ends with its last active pixel.
//
//   rtg_cli scene.xml --aov [--device N] [--seed S] [--out-dir DIR]
//
// --aov also writes every camera's first-hit feature images over its full sample range (rtg_render_aov):
// the shading normal as (n * 0.5 + 0.5) * 255, the albedo * 255 and the depth, named like the camera's image
// with _normal, _albedo and _depth before the extension.  One GPU, not with --progressive.
//
//   rtg_cli scene.xml --denoise [--aov] [--device N] [--seed S] [--out-dir DIR]
//
// --denoise also writes every camera's image filtered by the edge-avoiding denoiser (rtg_denoise), guided by those
// feature buffers and the per-pixel variance of a frame with moments, named with _denoised before the extension;
// the image files themselves are the ones a run without it writes, byte for byte.  One GPU, in one go: not with
// --progressive, --adaptive or --devices.
//
//   rtg_cli scene.xml --progressive K [--target-error E] --denoise-rounds ...
//
// --denoise-rounds (with --progressive) also rewrites the _denoised image after every round, filtered on the device
// from the round's frame (rtg_frame_denoise: the guides are traced once, nothing is downloaded but the result); the
// round lines and the camera's own files are those of --progressive alone.  Not with --adaptive, --devices, --aov
// or --denoise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rtg_host.h"

int main(int argc, char** argv) {
    const char* xml = nullptr;
    const char* out_dir = nullptr;
    int device = 0, devices = 0, progressive = 0;
    bool have_progressive = false, have_target = false;
    double target_error = 0.0, adaptive = 0.0;
    bool have_adaptive = false, have_min = false, aov = false, denoise = false, denoise_rounds = false;
    int min_samples = 2;
    unsigned long long seed = 0x5EED2026ull;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--devices") && i + 1 < argc) devices = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 0);
        else if (!strcmp(argv[i], "--out-dir") && i + 1 < argc) out_dir = argv[++i];
        else if (!strcmp(argv[i], "--progressive") && i + 1 < argc) { progressive = atoi(argv[++i]); have_progressive = true; }
        else if (!strcmp(argv[i], "--target-error") && i + 1 < argc) { target_error = atof(argv[++i]); have_target = true; }
        else if (!strcmp(argv[i], "--adaptive") && i + 1 < argc) { adaptive = atof(argv[++i]); have_adaptive = true; }
        else if (!strcmp(argv[i], "--min-samples") && i + 1 < argc) { min_samples = atoi(argv[++i]); have_min = true; }
        else if (!strcmp(argv[i], "--aov")) aov = true;
        else if (!strcmp(argv[i], "--denoise")) denoise = true;
        else if (!strcmp(argv[i], "--denoise-rounds")) denoise_rounds = true;
        else if (argv[i][0] == '-') { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        else xml = argv[i];
    }
    if (!xml) {
        fprintf(stderr, "usage: %s scene.xml [--device N] [--devices G] [--seed S] [--out-dir DIR] "
                        "[--progressive K [--target-error E | --adaptive REL [--min-samples M]] [--denoise-rounds]] [--aov] [--denoise]\n", argv[0]);
        return 2;
    }
    if (denoise_rounds && (!have_progressive || have_adaptive || devices > 0 || aov || denoise)) {
        fprintf(stderr, "rtg_cli: --denoise-rounds needs --progressive: it cannot be combined with --adaptive, --devices, "
                        "--aov or --denoise\n");
        return 2;
    }
    if (have_progressive && devices > 0) {
        fprintf(stderr, "rtg_cli: --progressive renders on one GPU: it cannot be combined with --devices\n");
        return 2;
    }
    if (aov && (have_progressive || devices > 0)) {
        fprintf(stderr, "rtg_cli: --aov renders on one GPU in one go: it cannot be combined with --devices or --progressive\n");
        return 2;
    }
    if (denoise && (have_progressive || have_adaptive || devices > 0)) {
        fprintf(stderr, "rtg_cli: --denoise renders on one GPU in one go: it cannot be combined with --devices, --progressive or --adaptive\n");
        return 2;
    }
    if ((have_progressive && progressive < 1) || (have_target && (!have_progressive || !(target_error >= 0.0)))) {
        fprintf(stderr, "rtg_cli: --progressive needs K >= 1, --target-error needs --progressive and E >= 0\n");
        return 2;
    }
    if ((have_adaptive && (!have_progressive || have_target || !(adaptive >= 0.0) || !(adaptive <= 3.0e38))) ||
        (have_min && (!have_adaptive || min_samples < 1))) {
        fprintf(stderr, "rtg_cli: --adaptive needs --progressive (without --target-error) and REL >= 0, "
                        "--min-samples needs --adaptive and M >= 1\n");
        return 2;
    }
    const int rc = have_adaptive ? rtgh_render_scene_adaptive(xml, device, seed, out_dir, progressive, adaptive, min_samples)
                 : denoise_rounds   ? rtgh_render_scene_progressive_denoise(xml, device, seed, out_dir, progressive, target_error)
                 : have_progressive ? rtgh_render_scene_progressive(xml, device, seed, out_dir, progressive, target_error)
                 : denoise          ? (aov ? rtgh_render_scene_denoise_aov(xml, device, seed, out_dir)
                                           : rtgh_render_scene_denoise(xml, device, seed, out_dir))
                 : aov              ? rtgh_render_scene_aov(xml, device, seed, out_dir)
                                    : rtgh_render_scene_multi(xml, device, devices, seed, out_dir);
    if (rc != RTG_OK) {
        fprintf(stderr, "rtg_cli: %s\n", rtgh_last_error());
        return 1;
    }
    return 0;
}
