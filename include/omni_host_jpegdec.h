/* omni_host_jpegdec.h -- C entry points of libomni_host_jpegdec.so (omni-swarm_amd/host/host_jpegdec_capi.cpp): is_compressed_images of the key-frame pipeline of
 * omni_host.h -- the camera frames arrive as JPEG files (sensor_msgs::CompressedImage; cv::imdecode(data, IMREAD_GRAYSCALE) in the reference, swarm_loop.cpp:72-89,
 * 291-292, 341-360) and are decoded on the GPU inside the key-frame unit, in front of the resize (csrc/jpeg_dec.hip).  STEREO_PINHOLE (left + right file per key
 * frame), PINHOLE_DEPTH (one file; the depth image stays uncompressed) and STEREO_FISHEYE in its raw-fisheye mode (omni_host_fisheye.h: the up and the down
 * fisheye frame as files).  A STEREO_FISHEYE pipeline fed flattened views and a pipeline attached to a sharded database ignore the switch.
 * The pixels are libjpeg-turbo's JCS_GRAYSCALE output, pinned against Pillow; parity with cv::imdecode itself is unpinned (OpenCV is not vendored).  The handle is
 * omni_host.h's omni_pipeline, whoever made it.  Returns as in omni_host.h: 0 on success; after a failure omni_jpegdec_host_last_error() holds the message (per
 * calling thread). */
#ifndef OMNI_HOST_JPEGDEC_H
#define OMNI_HOST_JPEGDEC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct omni_pipeline omni_pipeline;

const char* omni_jpegdec_host_last_error(void);

/* on != 0: every following key frame comes as JPEG files (omni_pipeline_push_keyframe_jpeg / omni_pipeline_run_jpeg); on == 0: as pixels (the default).  Refused
 * after the first key frame. */
int omni_pipeline_set_compressed_images(omni_pipeline* h, int on);
/* *on: the switch as set; *active: whether this pipeline's mode takes files (0 for STEREO_FISHEYE and under a sharded database) */
int omni_pipeline_get_compressed_images(omni_pipeline* h, int* on, int* active);
/* The text of the VINS settings file the node's vins_config_path names (OpenCV FileStorage YAML): the value of its is_compressed_images key (0 when absent, as the
 * reference's read of a missing node; *present tells).  omni_pipeline_apply_vins_settings sets the pipeline's switch from it (before the first key frame). */
int omni_swarm_vins_is_compressed_images(const char* vins_yaml_text, int* present);
int omni_pipeline_apply_vins_settings(omni_pipeline* h, const char* vins_yaml_text);
/* frames whose file could not be decoded so far (OMNI_JPEGDEC_CORRUPT): their pictures were all zeros -- no key points, landmark_num 0 */
int omni_pipeline_jpeg_corrupt(omni_pipeline* h, int64_t* count);
/* omni_pipeline_push_keyframe of omni_host.h for a key frame that comes as files: files[0] / sizes[0] the left (or only) frame, files[1] / sizes[1] the right one.
 * The files are copied before the call returns.  An UNSUPPORTED file (progressive, arithmetic, 12-bit) or a picture of another size than the pipeline's fails the
 * call that sends its unit to the GPU. */
int omni_pipeline_push_keyframe_jpeg(omni_pipeline* h, const uint8_t* const* files, const int64_t* sizes, int64_t msg_id, double stamp, const double* pose7,
                                     int prevent_adding_db, const uint16_t* depth, int* hits);
/* omni_pipeline_run of omni_host.h for n_keyframes key frames that come as files: key frame k's left (or only) file is files[cams * k], its right one
 * files[cams * k + 1] (cams = 2 for STEREO_PINHOLE, 1 for PINHOLE_DEPTH).  *hits += loop candidates found. */
int omni_pipeline_run_jpeg(omni_pipeline* h, int n_keyframes, int64_t first_msg_id, const uint8_t* const* files, const int64_t* sizes, int* hits);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_JPEGDEC_H */
