/* omni_host_jpeg.h -- C entry points of libomni_host_jpeg.so (omni-swarm_amd/host/host_jpeg_capi.cpp): send_img of the key-frame pipeline of omni_host.h --
 * the main image of every direction of a key frame as a JPEG file inside its message (encode_image, loop_cam.cpp:56-71, 306-308, 463-469), encoded inside the
 * key-frame unit on the GPU.  "Main image": the up camera's view of each direction (STEREO_FISHEYE), the left image (STEREO_PINHOLE), the one image
 * (PINHOLE_DEPTH).  The fisheye mask reaches the picture, as in the reference.  The bytes are libjpeg's defaults, pinned against Pillow (libjpeg-turbo); what
 * cv::imencode adds beyond them is unpinned (OpenCV is not vendored).  The handle is omni_host.h's omni_pipeline, whoever made it.  Returns as in omni_host.h:
 * 0 on success; after a failure omni_jpeg_host_last_error() holds the message (per calling thread). */
#ifndef OMNI_HOST_JPEG_H
#define OMNI_HOST_JPEG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct omni_pipeline omni_pipeline;

const char* omni_jpeg_host_last_error(void);

/* on != 0: every following key frame's main images are encoded at `quality` (1..100; the reference's jpg_quality, default 50) and stored in their messages;
 * on == 0: no image is encoded (the default, as the reference's).  Refused after the first key frame.  A pipeline attached to a sharded database builds no
 * messages: the call succeeds and nothing is encoded. */
int omni_pipeline_set_send_img(omni_pipeline* h, int on, int quality);
/* *on: the switch as set; *quality: jpg_quality; *active: whether images are encoded in this pipeline's mode (0 under a sharded database) */
int omni_pipeline_get_send_img(omni_pipeline* h, int* on, int* quality, int* active);
/* main images whose file exceeded the per-image capacity (width * height / 2) so far: their messages carry no image */
int omni_pipeline_jpeg_truncated(omni_pipeline* h, int64_t* count);
/* The JPEG stored with direction `direction` of key frame `msg_id` in the detector's database: *size = its bytes (0: no image), copied to out when
 * out != NULL and *size <= capacity.  Between two calls of run / push_keyframe / poll / flush only.  Fails for a key frame that is not in the database. */
int omni_pipeline_frame_image(omni_pipeline* h, int64_t msg_id, int direction, uint8_t* out, int64_t capacity, int64_t* size);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_JPEG_H */
