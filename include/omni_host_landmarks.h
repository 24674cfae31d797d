/* omni_host_landmarks.h -- C entry points of libomni_host_landmarks.so (omni-swarm_amd/host/host_landmarks_capi.cpp): where the key-frame pipeline of
 * omni_host.h computes the stereo landmarks of its key frames (generate_stereo_image_descriptor's lifting and triangulation, loop_cam.cpp:397-444).  The
 * handle is omni_host.h's omni_pipeline, whoever made it.  Returns as in omni_host.h: 0 on success; after a failure omni_landmarks_last_error() holds
 * the message (per calling thread). */
#ifndef OMNI_HOST_LANDMARKS_H
#define OMNI_HOST_LANDMARKS_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct omni_pipeline omni_pipeline;

const char* omni_landmarks_last_error(void);

/* on != 0: inside the key-frame unit, f64 on the GPU (the same arithmetic, bit for bit: csrc/landmark_plan.h), read back with the unit's results;
 * on == 0: on the host's geometry threads, after the unit's results have arrived.  Only a pipeline made with geometry != 0 and a stereo camera
 * configuration (STEREO_FISHEYE, STEREO_PINHOLE) computes stereo landmarks at all; elsewhere the call succeeds and changes nothing.  Refused after the
 * first key frame. */
int omni_pipeline_set_device_landmarks(omni_pipeline* h, int on);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_LANDMARKS_H */
