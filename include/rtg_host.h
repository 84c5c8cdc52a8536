/*
 * rtg_host.h — C ABI of the native host side (librtghost.so, raytracer-795_amd/host/):
 * the reference's Parser / Image / renderScene camera loop in C++ above include/rtg.h, so a
 * scene file goes from XML to images without Python (`rtg_cli scene.xml`, the reference's
 * `./raytracer scene.xml`, src/main.cpp:7-14).
 *
 *   rtgh_parse_xml      replaces  new Scene(xml) -> Parser::Parse* (src/Scene.cpp:455-504,
 *                                 src/Parser.h:17-1315) and yields the rtg_scene_desc that
 *                                 rtg_scene_create consumes, plus the cameras
 *   rtgh_save_image     replaces  Image::saveImage (src/Image.cpp:26-107: P3 text when the
 *                                 name contains ".png", else OpenEXR HALF via
 *                                 src/Helper.cpp:361-412)
 *   rtgh_render_scene   replaces  Scene::renderScene (src/Scene.cpp:294-363) end to end
 */
#ifndef RTG_HOST_H_
#define RTG_HOST_H_

#include "rtg.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtgh_scene rtgh_scene;

const char* rtgh_last_error(void);
/* Parse a CENG795 scene file (hw1-hw6 tags plus the hw7 <Renderer>, <RendererParams>,
   <LightSphere>, <LightMesh>).  PLY meshes and image textures are loaded relative to the
   XML's directory.  The descriptor stays valid until rtgh_free. */
int32_t rtgh_parse_xml(const char* xml_path, rtgh_scene** out);
const rtg_scene_desc* rtgh_scene_desc(const rtgh_scene* scene);
int32_t rtgh_num_cameras(const rtgh_scene* scene);
/* Camera i; image_name receives the <ImageName> (truncated to cap-1 bytes). */
int32_t rtgh_camera(const rtgh_scene* scene, int32_t i, rtg_camera_desc* out, char* image_name, int32_t cap);
/* Camera i's hw5 <Tonemap> (Photographic TMO): 1 and *out filled if present, 0 if not. */
int32_t rtgh_camera_tonemap(const rtgh_scene* scene, int32_t i, rtg_tonemap_desc* out);
void rtgh_free(rtgh_scene* scene);

/* Decode an image texture the way the reference's Texture constructor sees it
   (src/Texture.cpp:7-21, 41-74): *rgb = malloc'd ny*nx*3 floats [y][x][c], raw 0..255 for
   PNG/JPEG/PPM, linear floats for OpenEXR (LoadEXR's R,G,B, src/Helper.cpp:346-359).
   Release with rtgh_free_image. */
int32_t rtgh_read_image(const char* path, float** rgb, int32_t* nx, int32_t* ny);
void rtgh_free_image(float* rgb);

/* rgb: ny*nx*3 floats [y][x][c] (Image::_data). */
int32_t rtgh_save_image(const char* name, const float* rgb, int32_t nx, int32_t ny);

/* Parse, build on `device`, render every camera with Philox seed `seed`, save each image
   (under out_dir if not NULL/empty, else at its <ImageName>). */
int32_t rtgh_render_scene(const char* xml_path, int32_t device, uint64_t seed, const char* out_dir);
/* Same, every camera rendered on num_devices GPUs (device, device+1, ...): row-block shards,
   one host thread per GPU, RCCL gather of the rows (rtg_render_opts.num_devices / devices; with
   num_devices = 1 the one GPU is a one-rank RCCL job).  num_devices = 0: rtgh_render_scene. */
int32_t rtgh_render_scene_multi(const char* xml_path, int32_t device, int32_t num_devices, uint64_t seed,
                                const char* out_dir);
/* Progressive (rtg_frame, include/rtg.h): every camera is rendered in rounds of `step` samples.  After
   each round its image files are rewritten (the tone-mapped one too where the camera has a <Tonemap>)
   and one line goes to stdout: "<name>: <done>/<total> spp, mean_sem <s>, mean_luminance <l>".
   target_error > 0: a camera stops after the first round with mean_sem <= target_error *
   max(mean_luminance, FLT_MIN) and at least two samples (one sample has no
   variance).  Otherwise it runs to num_samples, and the final files are
   byte-identical to rtgh_render_scene's.
   (Declared `extern`: tests/test_host_native.py pins the twelve entry points above by their leading
   return type; tests/test_frame_abi.py checks that this one is exported.) */
extern int32_t rtgh_render_scene_progressive(const char* xml_path, int32_t device, uint64_t seed, const char* out_dir,
                                             int32_t step, double target_error);
/* Progressive with adaptive sampling (rtg_frame_retire): frames in sample order 1 with
   moments, rounds of `step` positions; after each round every pixel whose standard error is at most
   rel_tol x its mean luminance, and that holds at least max(min_samples, 2) samples, is retired and
   traced no further.  The round's line ends with ", active <pixels left>".  A camera ends with its last
   active pixel or its last sample.  (`extern` as above.) */
extern int32_t rtgh_render_scene_adaptive(const char* xml_path, int32_t device, uint64_t seed, const char* out_dir,
                                          int32_t step, double rel_tol, int32_t min_samples);
/* rtgh_render_scene with the first-hit feature images (rtg_render_aov over each camera's full sample
   range): beside a camera's image, three more through rtgh_save_image, named like it with
   _normal, _albedo and _depth before the extension: (normal * 0.5f + 0.5f) * 255.0f, albedo * 255.0f and
   the depth in all three channels.  (`extern` as above.) */
extern int32_t rtgh_render_scene_aov(const char* xml_path, int32_t device, uint64_t seed, const char* out_dir);
/* rtgh_render_scene with a denoised image per camera (rtg_denoise): every camera goes through
   one frame with moments whose samples are added in one go (the bits of rtg_render, so the image files are
   byte-identical to rtgh_render_scene's); its image, filtered under the first-hit guides of its full sample
   range with albedo demodulation and the variance of each pixel's mean luminance, is written through
   rtgh_save_image, named like the camera's image with _denoised before the extension.  A one-sample camera
   has no variance and is filtered without the luminance stop.  (`extern` as above.) */
extern int32_t rtgh_render_scene_denoise(const char* xml_path, int32_t device, uint64_t seed, const char* out_dir);
/* The same, and rtgh_render_scene_aov's three feature images from the same guides. */
extern int32_t rtgh_render_scene_denoise_aov(const char* xml_path, int32_t device, uint64_t seed, const char* out_dir);
/* rtgh_render_scene_progressive, and after every round the round's frame filtered on the device
   (rtg_frame_denoise with albedo demodulation, DESIGN.md §21: the guides are traced by the first round and kept,
   the variance is the frame's own) and written through rtgh_save_image, named like the camera's image with
   _denoised before the extension.  The per-round lines and the camera's own image files are those of
   rtgh_render_scene_progressive; run to num_samples, the last _denoised file is byte-identical to
   rtgh_render_scene_denoise's.  (`extern` as above.) */
extern int32_t rtgh_render_scene_progressive_denoise(const char* xml_path, int32_t device, uint64_t seed,
                                                     const char* out_dir, int32_t step, double target_error);

#ifdef __cplusplus
}
#endif
#endif /* RTG_HOST_H_ */
