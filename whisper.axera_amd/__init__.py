"""Python host mirror of the whisper.axera C ABI on MI355X (ctypes over libax_whisper.so).

The reference ships a Python twin of its C++ pipeline (python/whisper.py: ``Whisper(model_type,
model_path, language, task).run(audio)``); this module keeps that shape on top of the HIP
library. There is no CPU fallback: if the library or a GPU is missing, construction fails loudly.

The directory name contains a dot, so import it through the repo-root shim::

    import whisper_axera_amd as wa
    w = wa.Whisper("small", "/path/to/models", "zh")
    ids = w.run_tokens(pcm)
"""
from __future__ import annotations

import ctypes as C
import os
import re
import time
import subprocess
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libax_whisper.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ax_whisper_api.h")

fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int32)
_dblp = C.POINTER(C.c_double)
_lib = None
_cross_kv_env_lock = threading.Lock()  # Whisper(cross_kv=...): the variable is process-wide, one handle at a time is made under it

class LongOptions(C.Structure):
    """AX_WHISPER_LONG_OPTIONS"""
    _fields_ = [("no_speech_threshold", C.c_float), ("logprob_threshold", C.c_float), ("compression_ratio_threshold", C.c_float),
                ("temperatures", fp), ("n_temperatures", C.c_int), ("seed", C.c_uint64), ("file_ids", C.POINTER(C.c_int)),
                ("initial_prompt_ids", ip), ("prompt_stride", C.c_int), ("n_initial", C.POINTER(C.c_int)), ("condition_on_previous_text", C.c_int),
                ("lang", C.POINTER(C.c_int)), ("task", C.POINTER(C.c_int)), ("word_timestamps", C.c_int)]


class ChunkOptions(C.Structure):
    """AX_WHISPER_CHUNK_OPTIONS"""
    _fields_ = [("max_frames", C.c_int), ("min_frames", C.c_int), ("smooth_frames", C.c_int), ("beam_size", C.c_int)]


class LongWordLog(C.Structure):
    """AX_WHISPER_LONG_WORD_LOG"""
    _fields_ = [("seg_cap", C.c_int), ("word_cap", C.c_int), ("win_words", C.POINTER(C.c_int)), ("text_ids", ip), ("jump", C.POINTER(C.c_int)),
                ("token_logprob", fp), ("seg_tokens", C.POINTER(C.c_int)), ("seg_start", _dblp), ("seg_end", _dblp),
                ("word_segment", C.POINTER(C.c_int)), ("word_text_end", C.POINTER(C.c_int)), ("word_start", _dblp), ("word_end", _dblp),
                ("word_prob", fp), ("text", C.c_void_p)]


class LongWords(C.Structure):
    """AX_WHISPER_LONG_WORDS"""
    _fields_ = [("n_segments", C.c_int), ("n_words", C.c_int), ("seg_start", _dblp), ("seg_end", _dblp), ("seg_text_end", C.POINTER(C.c_int)),
                ("seg_text", C.c_void_p), ("word_segment", C.POINTER(C.c_int)), ("word_start", _dblp), ("word_end", _dblp), ("word_prob", fp),
                ("word_text_end", C.POINTER(C.c_int)), ("word_text", C.c_void_p)]


# name -> (restype, argtypes): every symbol include/ax_whisper_api.h declares
SYMBOLS = {
    "AX_WHISPER_Init": (C.c_void_p, [C.c_char_p, C.c_char_p, C.c_char_p]),
    "AX_WHISPER_InitEx": (C.c_void_p, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]),
    "AX_WHISPER_InitMulti": (C.c_void_p, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_int]),
    "AX_WHISPER_GetDeviceCount": (C.c_int, [C.c_void_p]),
    "AX_WHISPER_VisibleDeviceCount": (C.c_int, []),
    "AX_WHISPER_Uninit": (None, [C.c_void_p]),
    "AX_WHISPER_RunFile": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunPCM": (C.c_int, [C.c_void_p, fp, C.c_int, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_GetConfigInt": (C.c_int, [C.c_void_p, C.c_char_p]),
    "AX_WHISPER_LastError": (C.c_char_p, [C.c_void_p]),
    "AX_WHISPER_SetStream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "AX_WHISPER_RunPCMBatchTokens": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMBatch": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunDeviceBatchTokens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_RunDeviceBatchTokensRagged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_Detokenize": (C.c_int, [C.c_void_p, ip, C.c_int, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_Transcript": (C.c_int, [C.c_void_p, ip, C.c_int, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_ConvertT2S": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_LoadAudioFile": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_DetokenizeWithTable": (C.c_int, [C.c_char_p, ip, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "AX_WHISPER_ComputeMel": (C.c_int, [C.c_void_p, fp, C.c_int, fp]),
    "AX_WHISPER_EncodeMel": (C.c_int, [C.c_void_p, fp, C.c_int]),
    "AX_WHISPER_GetCrossKV": (C.c_int, [C.c_void_p, C.c_int, fp, fp]),
    "AX_WHISPER_GetCrossKVFp8": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), fp]),
    "AX_WHISPER_CrossKVQuantize": (C.c_int, [C.c_void_p]),
    "AX_WHISPER_ScanStored16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int64), fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_DecodeForced": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, fp, ip]),
    "AX_WHISPER_DecodeGreedy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_DecodeGreedyRagged": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_StreamOpen": (C.c_int, [C.c_void_p, C.c_int]),
    "AX_WHISPER_StreamAdmit": (C.c_int, [C.c_void_p, C.c_int, fp, C.c_int, C.c_int]),
    "AX_WHISPER_StreamAdmitBatch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(fp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "AX_WHISPER_StreamStep": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_StreamCollect": (C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_StreamClose": (C.c_int, [C.c_void_p]),
    "AX_WHISPER_GetTimings": (C.c_int, [C.c_void_p, fp]),
    "AX_WHISPER_Bench": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, fp]),
    "AX_WHISPER_RunPCMBatchTimestampTokens": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_DecodeForcedTimestamps": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, fp, ip]),
    "AX_WHISPER_ApplyTimestampRules": (C.c_int, [C.c_void_p, fp, ip, C.POINTER(C.c_int), C.c_int, ip]),
    "AX_WHISPER_SplitSegments": (C.c_int, [ip, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, fp, fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_SplitWindow": (C.c_int, [ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_ComputeMelWindow": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_int, fp]),
    "AX_WHISPER_RunPCMLongWindows": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLong": (C.c_int, [C.c_void_p, fp, C.c_int, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunFileLong": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunPCMBatchTimestampScores": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), ip, C.POINTER(C.c_int), fp, fp, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_DecodeForcedTimestampScores": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, fp, ip, fp, fp, fp]),
    "AX_WHISPER_ScoreTimestampRules": (C.c_int, [C.c_void_p, fp, ip, C.POINTER(C.c_int), C.c_int, ip, fp]),
    "AX_WHISPER_NoSpeechLogProb": (C.c_int, [C.c_void_p, fp, C.c_int, fp]),
    "AX_WHISPER_LongWindowIsSilent": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float]),
    "AX_WHISPER_RunPCMLongWindowsScored": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int), ip, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLongOpts": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunFileLongOpts": (C.c_int, [C.c_void_p, C.c_char_p, C.c_float, C.c_float, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_SampleTimestampRules": (C.c_int, [C.c_void_p, fp, ip, C.POINTER(C.c_int), C.c_int, fp, C.POINTER(C.c_uint64), C.c_uint64, ip, fp]),
    "AX_WHISPER_DecodeForcedTimestampSampled": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, fp, C.POINTER(C.c_uint64), C.c_uint64, fp, ip, fp, fp, fp]),
    "AX_WHISPER_RunPCMBatchTimestampSampled": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), fp, C.POINTER(C.c_uint64), C.c_uint64, ip, C.POINTER(C.c_int), fp, fp, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_CompressionRatio": (C.c_int, [C.c_char_p, C.c_int, fp]),
    "AX_WHISPER_WindowNeedsFallback": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "AX_WHISPER_RunPCMLongWindowsFallback": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), ip, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLongFallback": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunFileLongFallback": (C.c_int, [C.c_void_p, C.c_char_p, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunPCMBatchBeam": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, ip, C.POINTER(C.c_int), fp, fp, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_DecodeBeam": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, C.POINTER(C.c_int), fp, fp, fp, C.POINTER(C.c_int),
                                        ip, C.POINTER(C.c_int), fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.c_int, fp, ip, fp, C.POINTER(C.c_int), fp, C.POINTER(C.c_int), C.POINTER(C.c_int), ip, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_BeamCandidates": (C.c_int, [C.c_void_p, fp, ip, C.POINTER(C.c_int), C.c_int, C.c_int, ip, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_BeamSelect": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, fp, C.POINTER(C.c_int), ip,
                                        fp, C.POINTER(C.c_int), C.POINTER(C.c_int), ip, C.POINTER(C.c_int), fp, C.POINTER(C.c_int), ip, C.POINTER(C.c_int), fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_BeamFinalize": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, ip, fp, C.POINTER(C.c_int), C.POINTER(C.c_int), ip, C.POINTER(C.c_int), fp,
                                          ip, C.POINTER(C.c_int), fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), ip, C.POINTER(C.c_int), fp, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMBatchTimestampPrompted": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), ip, C.c_int, C.POINTER(C.c_int), ip, C.POINTER(C.c_int), fp, fp, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_PrefillPrompts": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, C.POINTER(C.c_int), fp, fp]),
    "AX_WHISPER_GetSelfKV": (C.c_int, [C.c_void_p, C.c_int, C.c_int, fp, fp]),
    "AX_WHISPER_GetPersistentSelfKV": (C.c_int, [C.c_void_p, C.c_int, fp, fp]),
    "AX_WHISPER_DecodeForcedTimestampPrompted": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, C.POINTER(C.c_int), ip, C.c_int, fp, ip, fp, fp]),
    "AX_WHISPER_CarryPrompt": (C.c_int, [ip, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, ip,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLongWindowsPrompted": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, C.POINTER(C.c_int),
                                                       ip, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), ip, fp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLongPrompted": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, ip, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunFileLongPrompted": (C.c_int, [C.c_void_p, C.c_char_p, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, ip, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_LanguageIndex": (C.c_int, [C.c_void_p, C.c_char_p]),
    "AX_WHISPER_LanguageCode": (C.c_char_p, [C.c_void_p, C.c_int]),
    "AX_WHISPER_DetectLanguage": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), fp]),
    "AX_WHISPER_RunPCMBatchTimestampLang": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), ip, C.c_int, C.POINTER(C.c_int),
                                                      C.POINTER(C.c_int), C.POINTER(C.c_int), ip, C.POINTER(C.c_int), fp, fp, fp, C.POINTER(C.c_int), C.POINTER(C.c_int), fp]),
    "AX_WHISPER_DetectLanguageStage": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), fp, fp]),
    "AX_WHISPER_LanguageLogProbRows": (C.c_int, [C.c_void_p, fp, C.c_int, fp, C.POINTER(C.c_int), fp]),
    "AX_WHISPER_PrefillContexts": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), fp, fp, C.POINTER(C.c_int), fp]),
    "AX_WHISPER_DecodeForcedTimestampLang": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), ip, C.c_int, fp, ip, fp, fp,
                                                       C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLongWindowsLang": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, C.POINTER(C.c_int),
                                                   ip, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), ip, fp, C.POINTER(C.c_int),
                                                   C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLongLang": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunFileLongLang": (C.c_int, [C.c_void_p, C.c_char_p, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_uint64, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "AX_WHISPER_TranscriptLang": (C.c_int, [C.c_void_p, ip, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_PersistentDecodePlan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMBatchWordTimestamps": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), ip,
                                                       C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), _dblp, _dblp, C.POINTER(C.c_int),
                                                       C.POINTER(C.c_int), C.POINTER(C.c_int), _dblp, _dblp, fp, C.POINTER(C.c_void_p), C.POINTER(C.c_int), fp]),
    "AX_WHISPER_AlignTokens": (C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), fp, fp, C.c_int, C.c_int]),
    "AX_WHISPER_VocabLogProbRows": (C.c_int, [C.c_void_p, fp, C.c_int, ip, fp, C.c_int]),
    "AX_WHISPER_VocabLogProbPlan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "AX_WHISPER_SetAlignmentHeads": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "AX_WHISPER_ConfigAlignmentHeads": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_SetSuppressTokens": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "AX_WHISPER_GetSuppressTokens": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_NonSpeechTokens": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_ConfigSuppressTokens": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_AlignQKSoftmax": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), fp, C.c_int, C.c_int, C.POINTER(C.c_int), fp, C.c_int,
                                            C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, fp, C.c_int, C.c_int]),
    "AX_WHISPER_AlignNormalize": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), fp, C.c_int, C.c_int, C.c_int, C.c_float, fp, C.c_int,
                                            C.c_int]),
    "AX_WHISPER_AlignDTW": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), fp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "AX_WHISPER_AlignPath": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "AX_WHISPER_SplitWords": (C.c_int, [C.c_char_p, ip, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "AX_WHISPER_WordsFromAlignment": (C.c_int, [C.c_char_p, ip, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int), _dblp, _dblp, C.c_int, C.POINTER(C.c_int), fp,
                                                C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _dblp, _dblp, fp, C.POINTER(C.c_int),
                                                C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "AX_WHISPER_WordsFromAlignmentAt": (C.c_int, [C.c_char_p, ip, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int), _dblp, _dblp, C.c_int, C.POINTER(C.c_int), fp,
                                                  C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _dblp, _dblp, fp, C.POINTER(C.c_int),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "AX_WHISPER_LongWordAdvance": (C.c_int, [ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLongWindowsWords": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(LongOptions), C.c_int,
                                                    C.POINTER(C.c_int), ip, fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                    C.POINTER(LongWordLog)]),
    "AX_WHISPER_RunPCMLongWords": (C.c_int, [C.c_void_p, fp, C.c_int, C.POINTER(LongOptions), C.POINTER(C.c_int), C.POINTER(LongWords)]),
    "AX_WHISPER_RunFileLongWords": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(LongOptions), C.POINTER(C.c_int), C.POINTER(LongWords)]),
    "AX_WHISPER_FreeLongWords": (None, [C.POINTER(LongWords)]),
    "AX_WHISPER_ResampledLength": (C.c_longlong, [C.c_longlong, C.c_int]),
    "AX_WHISPER_ResampleFilter": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), fp, C.c_int]),
    "AX_WHISPER_ResampleBatch": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(fp), C.POINTER(C.c_int),
                                           C.POINTER(C.c_int)]),
    "AX_WHISPER_ComputeMelRate": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_int, fp]),
    "AX_WHISPER_RunPCMBatchRate": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(fp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, ip, C.POINTER(C.c_int)]),
    "AX_WHISPER_StreamAdmitBatchRate": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(fp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "AX_WHISPER_RunFileResampled": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "AX_WHISPER_LoadAudioFile16k": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_LongCutPlanHost": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_ChunkedSegments": (C.c_int, [ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dblp, _dblp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int)]),
    "AX_WHISPER_LongFrameLevels": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(fp), C.POINTER(fp)]),
    "AX_WHISPER_LongCutPlanFromLevels": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "AX_WHISPER_LongCutPlan": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.POINTER(ChunkOptions), C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(fp)]),
    "AX_WHISPER_ComputeMelWindowCut": (C.c_int, [C.c_void_p, fp, C.c_int, C.c_int, C.c_int, fp]),
    "AX_WHISPER_RunPCMLongChunkedWindows": (C.c_int, [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(ChunkOptions),
                                                      C.POINTER(LongOptions), C.c_int, C.POINTER(C.c_int), ip, fp, C.POINTER(C.c_int)]),
    "AX_WHISPER_RunPCMLongChunked": (C.c_int, [C.c_void_p, fp, C.c_int, C.POINTER(ChunkOptions), C.POINTER(LongOptions), C.POINTER(C.c_void_p)]),
    "AX_WHISPER_RunFileLongChunked": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(ChunkOptions), C.POINTER(LongOptions), C.POINTER(C.c_void_p)]),
    "AX_WHISPER_StreamOpenMode": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "AX_WHISPER_StreamAdmitBatchLang": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(fp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "AX_WHISPER_StreamCollectScored": (C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(C.c_int), fp, fp, fp, C.POINTER(C.c_int), C.POINTER(C.c_int), fp]),
    "AX_WHISPER_StreamRulesStage": (C.c_int, [C.c_void_p, C.c_int, fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), ip, C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), ip, fp, fp, C.POINTER(C.c_int), fp]),
}


def build(verbose: bool = False) -> str:
    """Compile libax_whisper.so, whisper_cli and whisper_srv for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", _HERE, "-j8"], capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libax_whisper.so failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


def load_library():
    """dlopen the HIP library; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (the engine has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        L._free = C.CDLL(None).free
        L._free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def convert_t2s(config_path: str, text: str) -> str:
    """The reference's zh post-pass on its own (cpp/src/Whisper.cpp:231-236): OpenCC t2s.json + its .ocd2 dictionaries."""
    L = load_library()
    out = C.c_void_p()
    if L.AX_WHISPER_ConvertT2S(os.fspath(config_path).encode(), text.encode("utf-8"), C.byref(out)) != 0:
        raise RuntimeError("AX_WHISPER_ConvertT2S failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    s = C.string_at(out.value).decode("utf-8")
    L._free(out.value)
    return s


def load_audio_file(path: str):
    """The file decode of AX_WHISPER_RunFile on its own (host only) -> (mono f32 samples, sample rate, channels)."""
    L = load_library()
    out, n, info = C.c_void_p(), C.c_int(), (C.c_int * 2)()
    if L.AX_WHISPER_LoadAudioFile(os.fspath(path).encode(), C.byref(out), C.byref(n), info) != 0:
        raise RuntimeError("AX_WHISPER_LoadAudioFile failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    a = np.ctypeslib.as_array(C.cast(out, fp), shape=(max(n.value, 1),))[: n.value].copy()
    L._free(out.value)
    return a, info[0], info[1]


def resampled_length(n: int, rate: int) -> int:
    """The length at 16 kHz of a clip of n samples at `rate` Hz, ceil(n * 16000 / rate) (host only); raises on a refused rate or length."""
    L = load_library()
    r = L.AX_WHISPER_ResampledLength(int(n), int(rate))
    if r < 0:
        raise ValueError("AX_WHISPER_ResampledLength: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    return int(r)


def resample_filter(rate: int):
    """The polyphase filter of `rate` as the resample kernel uses it (host only) -> (L, M, K, table float32 [L][2 K])."""
    L = load_library()
    l, m, k = C.c_int(), C.c_int(), C.c_int()
    if L.AX_WHISPER_ResampleFilter(int(rate), C.byref(l), C.byref(m), C.byref(k), None, 0) != 0:
        raise ValueError("AX_WHISPER_ResampleFilter: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    table = np.empty((l.value, 2 * k.value), dtype=np.float32)
    if L.AX_WHISPER_ResampleFilter(int(rate), C.byref(l), C.byref(m), C.byref(k), table.ctypes.data_as(fp), table.size) != 0:
        raise ValueError("AX_WHISPER_ResampleFilter: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    return l.value, m.value, k.value, table


def detokenize_with_table(tokens_path: str, ids) -> bytes:
    """ids -> bytes through a tokens file alone (host only): what Whisper.detokenize returns for them."""
    L = load_library()
    a = np.ascontiguousarray(ids, dtype=np.int32)
    out, n = C.c_void_p(), C.c_int()
    if L.AX_WHISPER_DetokenizeWithTable(os.fspath(tokens_path).encode(), a.ctypes.data_as(ip), len(a), C.byref(out), C.byref(n)) != 0:
        raise RuntimeError("AX_WHISPER_DetokenizeWithTable failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    b = C.string_at(out.value, n.value)
    L._free(out.value)
    return b


def split_segments(ids, timestamp_begin: int, eot: int, clip_seconds: float):
    """One clip's timestamp-mode ids (eot excluded) -> [(start_s, end_s, tok_begin, tok_end)] (AX_WHISPER_SplitSegments, host
    only): ids[tok_begin:tok_end] are the segment's text ids."""
    L = load_library()
    a = np.ascontiguousarray(ids, dtype=np.int32)
    n_max = len(a) // 2 + 1
    st, en = np.zeros(n_max, dtype=np.float32), np.zeros(n_max, dtype=np.float32)
    tb, te = np.zeros(n_max, dtype=np.int32), np.zeros(n_max, dtype=np.int32)
    n = C.c_int()
    pi = C.POINTER(C.c_int)
    if L.AX_WHISPER_SplitSegments(a.ctypes.data_as(ip), len(a), int(timestamp_begin), int(eot), float(clip_seconds), n_max,
                                  st.ctypes.data_as(fp), en.ctypes.data_as(fp), tb.ctypes.data_as(pi), te.ctypes.data_as(pi), C.byref(n)) != 0:
        raise RuntimeError("AX_WHISPER_SplitSegments failed")
    return [(float(st[k]), float(en[k]), int(tb[k]), int(te[k])) for k in range(n.value)]


def split_window(ids, timestamp_begin: int, eot: int, window_frames: int):
    """The long-form window rule (AX_WHISPER_SplitWindow, host only): one window's ids (eot excluded) ->
    ([(start_s, end_s, tok_begin, tok_end)] relative to the window, advance in frames of 10 ms)."""
    L = load_library()
    a = np.ascontiguousarray(ids, dtype=np.int32)
    n_max = len(a) // 2 + 1
    st, en = np.zeros(n_max, dtype=np.float32), np.zeros(n_max, dtype=np.float32)
    tb, te = np.zeros(n_max, dtype=np.int32), np.zeros(n_max, dtype=np.int32)
    n, adv = C.c_int(), C.c_int()
    pi = C.POINTER(C.c_int)
    if L.AX_WHISPER_SplitWindow(a.ctypes.data_as(ip), len(a), int(timestamp_begin), int(eot), int(window_frames), n_max,
                                st.ctypes.data_as(fp), en.ctypes.data_as(fp), tb.ctypes.data_as(pi), te.ctypes.data_as(pi),
                                C.byref(n), C.byref(adv)) != 0:
        raise RuntimeError("AX_WHISPER_SplitWindow failed")
    return [(float(st[k]), float(en[k]), int(tb[k]), int(te[k])) for k in range(n.value)], adv.value


def long_cut_plan_host(s, min_frames: int = 2000, max_frames: int = 3000, content=None):
    """The cut rule of chunked long-form on levels s (AX_WHISPER_LongCutPlanHost, host only) -> [(seek, len)]. content: frames of
    audio (default: len(s)). Raises ValueError on refused parameters or non-finite levels."""
    L = load_library()
    a = _f32(s)
    content = len(a) if content is None else int(content)
    if content > len(a):
        raise ValueError("content beyond the levels")
    cap = content // max(int(min_frames), 1) + 2
    seek, ln, n = (C.c_int * cap)(), (C.c_int * cap)(), C.c_int()
    if L.AX_WHISPER_LongCutPlanHost(a.ctypes.data_as(fp), content, int(min_frames), int(max_frames), cap, seek, ln, C.byref(n)) != 0:
        raise ValueError("AX_WHISPER_LongCutPlanHost: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    return [(seek[k], ln[k]) for k in range(n.value)]


def chunked_segments(ids, timestamp_begin: int, eot: int, seek: int, length: int):
    """One window's ids (eot excluded) of chunked long-form -> [(start_s, end_s, tok_begin, tok_end)] in FILE time
    (AX_WHISPER_ChunkedSegments, host only)."""
    L = load_library()
    a = np.ascontiguousarray(ids, dtype=np.int32)
    n_max = len(a) // 2 + 1
    st, en = np.zeros(n_max, dtype=np.float64), np.zeros(n_max, dtype=np.float64)
    tb, te = np.zeros(n_max, dtype=np.int32), np.zeros(n_max, dtype=np.int32)
    n = C.c_int()
    pi = C.POINTER(C.c_int)
    if L.AX_WHISPER_ChunkedSegments(a.ctypes.data_as(ip), len(a), int(timestamp_begin), int(eot), int(seek), int(length), n_max,
                                    st.ctypes.data_as(_dblp), en.ctypes.data_as(_dblp), tb.ctypes.data_as(pi), te.ctypes.data_as(pi), C.byref(n)) != 0:
        raise RuntimeError("AX_WHISPER_ChunkedSegments failed")
    return [(float(st[k]), float(en[k]), int(tb[k]), int(te[k])) for k in range(n.value)]


def long_window_is_silent(no_speech_logprob: float, avg_logprob: float, no_speech_threshold: float, logprob_threshold: float) -> bool:
    """The silent-window rule of the long-form loop (AX_WHISPER_LongWindowIsSilent, host only): exp(no_speech_logprob) >
    no_speech_threshold and not avg_logprob > logprob_threshold, in float32."""
    L = load_library()
    return bool(L.AX_WHISPER_LongWindowIsSilent(float(no_speech_logprob), float(avg_logprob), float(no_speech_threshold), float(logprob_threshold)))


DEFAULT_TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)  # openai-whisper's


def compression_ratio(data) -> float:
    """len(bytes) / len(zlib.compress(bytes)) (AX_WHISPER_CompressionRatio, host only); str is taken as UTF-8."""
    L = load_library()
    b = data.encode("utf-8") if isinstance(data, str) else bytes(data)
    out = C.c_float()
    if L.AX_WHISPER_CompressionRatio(b, len(b), C.byref(out)) != 0:
        raise RuntimeError("AX_WHISPER_CompressionRatio failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    return out.value


def window_needs_fallback(compression_ratio: float, avg_logprob: float, no_speech_logprob: float, compression_ratio_threshold=None,
                          logprob_threshold=None, no_speech_threshold=None) -> bool:
    """openai-whisper's fallback rule (AX_WHISPER_WindowNeedsFallback, host only); None switches a threshold's part off."""
    L = load_library()
    nan = lambda v: float("nan") if v is None else float(v)
    return bool(L.AX_WHISPER_WindowNeedsFallback(float(compression_ratio), float(avg_logprob), float(no_speech_logprob),
                                                 nan(compression_ratio_threshold), nan(logprob_threshold), nan(no_speech_threshold)))


def carry_prompt(all_ids, reset_since: int, window_ids, timestamp_begin: int, eot: int, window_frames: int, skipped: bool = False,
                 condition_on_previous_text: bool = True, temperature: float = 0.0, keep: int = 223):
    """One step of the previous-text carry after a kept window (AX_WHISPER_CarryPrompt, host only) ->
    (all_ids, reset_since, n_prompt_next): the next window's prompt is all_ids[reset_since:][-keep:]."""
    L = load_library()
    a, w = _i32(all_ids), _i32(window_ids)
    cap = len(a) + len(w)
    out = np.zeros(max(cap, 1), dtype=np.int32)
    n, rs, npn = C.c_int(), C.c_int(), C.c_int()
    if L.AX_WHISPER_CarryPrompt(a.ctypes.data_as(ip), len(a), int(reset_since), w.ctypes.data_as(ip), len(w), int(timestamp_begin), int(eot),
                                int(window_frames), int(bool(skipped)), int(bool(condition_on_previous_text)), float(temperature), int(keep), cap,
                                out.ctypes.data_as(ip), C.byref(n), C.byref(rs), C.byref(npn)) != 0:
        raise RuntimeError("AX_WHISPER_CarryPrompt failed")
    return out[: n.value].tolist(), rs.value, npn.value


def persistent_decode_plan(d_model: int, n_head: int, n_layer: int, n_cu: int, n_clips: int = 0, t0: int = 0, n_slots: int = 0):
    """The decode path Init picks for a decoder shape on n_cu compute units (AX_WHISPER_PersistentDecodePlan, host only) ->
    dict(grid, supported, max_clips, free_workgroups); with n_clips > 0 also units: int32 [n_slots][grid], the cross-attention
    unit (or -1) of every workgroup in layer slots t0 .. t0 + n_slots - 1 of an n_clips launch."""
    L = load_library()
    plan = (C.c_int * 4)()
    units = None
    if n_clips > 0:
        if L.AX_WHISPER_PersistentDecodePlan(d_model, n_head, n_layer, n_cu, 0, 0, 0, plan, None) != 0:
            raise RuntimeError("AX_WHISPER_PersistentDecodePlan failed")
        units = np.empty((n_slots, plan[0]), dtype=np.int32)
    if L.AX_WHISPER_PersistentDecodePlan(d_model, n_head, n_layer, n_cu, n_clips, t0, n_slots, plan,
                                         units.ctypes.data_as(C.POINTER(C.c_int)) if units is not None else None) != 0:
        raise RuntimeError("AX_WHISPER_PersistentDecodePlan failed")
    out = dict(grid=plan[0], supported=bool(plan[1]), max_clips=plan[2], free_workgroups=plan[3])
    if units is not None:
        out["units"] = units
    return out


def _thresholds(no_speech_threshold, logprob_threshold):
    """None -> the values that switch a comparison off: NaN (never silent) / +inf (no-speech alone decides)."""
    return (float("nan") if no_speech_threshold is None else float(no_speech_threshold),
            float("inf") if logprob_threshold is None else float(logprob_threshold))


def _long_fallback_args(o):
    return (o.no_speech_threshold, o.logprob_threshold, o.compression_ratio_threshold, o.temperatures, o.n_temperatures, o.seed)


def _long_prompted_args(o):
    return _long_fallback_args(o) + (o.file_ids, o.initial_prompt_ids, o.prompt_stride, o.n_initial, o.condition_on_previous_text)


def _long_text_prompted_args(o):
    return _long_fallback_args(o) + (o.initial_prompt_ids, o.n_initial[0], o.condition_on_previous_text)


# The legacy argument lists of the long-form exports, each a part of a LongOptions `o`: the form (what follows RunPCMLongWindows in the
# export's name) -> the arguments between the files and the outputs. The one-file text forms (RunPCMLong<form> / RunFileLong<form>)
# take one prompt, one language and one task by value and no file ids; their last None is lang_out.
_LONG_FORMS = {"": lambda o: (), "Scored": lambda o: (o.no_speech_threshold, o.logprob_threshold),
               "Fallback": lambda o: _long_fallback_args(o) + (o.file_ids,), "Prompted": _long_prompted_args,
               "Lang": lambda o: _long_prompted_args(o) + (o.lang, o.task), "Words": lambda o: (C.byref(o),)}
_LONG_TEXT_FORMS = {"": lambda o: (), "Opts": _LONG_FORMS["Scored"], "Fallback": _long_fallback_args, "Prompted": _long_text_prompted_args,
                    "Lang": lambda o: _long_text_prompted_args(o) + (o.lang[0] if o.lang else -1, o.task[0] if o.task else 0, None)}


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


_cip = C.POINTER(C.c_int)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ci(a):
    """int32 array -> the `int*` of the C ABI"""
    return a.ctypes.data_as(_cip)


def _word_texts(L, out, n_bytes, text_end, n):
    """the malloc'ed bytes of n words, word w ending at byte text_end[w] -> [bytes]; frees the buffer"""
    b = C.string_at(out.value, n_bytes) if out.value else b""
    if out.value:
        L._free(out.value)
    ends = [0] + [int(e) for e in text_end[:n]]
    return [b[ends[w]: ends[w + 1]] for w in range(n)]


def config_alignment_heads(config_path: str):
    """Host only (AX_WHISPER_ConfigAlignmentHeads): the [(layer, head)] a handle constructed from this {type}_config.json starts
    with: its "alignment_heads" key, else every head of the upper half of the decoder layers."""
    L = load_library()
    n_max = 4096
    pairs, n = np.zeros(2 * n_max, dtype=np.int32), C.c_int()
    if L.AX_WHISPER_ConfigAlignmentHeads(os.fspath(config_path).encode(), n_max, _ci(pairs), C.byref(n)) != 0:
        raise RuntimeError("AX_WHISPER_ConfigAlignmentHeads failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    return [(int(pairs[2 * i]), int(pairs[2 * i + 1])) for i in range(n.value)]


def non_speech_tokens(tokens_path: str):
    """Host only (AX_WHISPER_NonSpeechTokens): the sorted ids that openai-whisper's suppress_tokens = -1 stands for, derived from a
    {type}-tokens.txt (DESIGN.md "Token suppression")."""
    L = load_library()
    n_max = 4096
    ids, n = np.zeros(n_max, dtype=np.int32), C.c_int()
    if L.AX_WHISPER_NonSpeechTokens(os.fspath(tokens_path).encode(), n_max, _ci(ids), C.byref(n)) != 0:
        raise RuntimeError("AX_WHISPER_NonSpeechTokens failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    return [int(x) for x in ids[: n.value]]


def config_suppress_tokens(config_path: str, tokens_path: str = None):
    """Host only (AX_WHISPER_ConfigSuppressTokens): the sorted suppress set a handle constructed from this {type}_config.json starts
    with: its "suppress_tokens" key, an entry -1 standing for non_speech_tokens(tokens_path); absent or []: none."""
    L = load_library()
    n_max = 1 << 17
    ids, n = np.zeros(n_max, dtype=np.int32), C.c_int()
    tp = os.fspath(tokens_path).encode() if tokens_path is not None else None
    if L.AX_WHISPER_ConfigSuppressTokens(os.fspath(config_path).encode(), tp, n_max, _ci(ids), C.byref(n)) != 0:
        raise RuntimeError("AX_WHISPER_ConfigSuppressTokens failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    return [int(x) for x in ids[: n.value]]


def vocab_logprob_plan(d_model: int, n_rows: int, eot: int):
    """Host only (AX_WHISPER_VocabLogProbPlan): the fused log-prob kernel's tiling -> (rows per row tile, vocabulary splits,
    columns per split)."""
    L = load_library()
    plan = (C.c_int * 3)()
    if L.AX_WHISPER_VocabLogProbPlan(int(d_model), int(n_rows), int(eot), plan) != 0:
        raise ValueError("AX_WHISPER_VocabLogProbPlan: a shape the kernel does not take")
    return plan[0], plan[1], plan[2]


def align_path(matrix) -> np.ndarray:
    """Host only (AX_WHISPER_AlignPath): matrix [rows][frames] -> jump [rows], the frame of the first point of every row on the
    DTW path over -matrix (fp32 accumulation, ties go left)."""
    L = load_library()
    m = _f32(matrix)
    if m.ndim != 2:
        raise ValueError("a [rows][frames] matrix")
    jump = np.zeros(m.shape[0], dtype=np.int32)
    if L.AX_WHISPER_AlignPath(m.ctypes.data_as(fp), m.shape[0], m.shape[1], m.shape[1], _ci(jump)) != 0:
        raise RuntimeError("AX_WHISPER_AlignPath failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    return jump


def split_words(tokens_path: str, ids, eot: int, language: str):
    """Host only (AX_WHISPER_SplitWords): openai-whisper's split_to_word_tokens -> [(word bytes, [ids])]."""
    L = load_library()
    a = _i32(ids).reshape(-1)
    n_max = max(len(a), 1)
    wt, te = np.zeros(n_max, dtype=np.int32), np.zeros(n_max, dtype=np.int32)
    n, nb, out = C.c_int(), C.c_int(), C.c_void_p()
    if L.AX_WHISPER_SplitWords(os.fspath(tokens_path).encode(), a.ctypes.data_as(ip), len(a), int(eot), language.encode(), n_max, _ci(wt), _ci(te),
                               C.byref(n), C.byref(out), C.byref(nb)) != 0:
        raise RuntimeError("AX_WHISPER_SplitWords failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    texts = _word_texts(L, out, nb.value, te, n.value)
    ends = np.concatenate([[0], np.cumsum(wt[: n.value])])
    return [(texts[w], a[ends[w]: ends[w + 1]].tolist()) for w in range(n.value)]


def long_word_advance(ids, timestamp_begin: int, seek: int, window_frames: int, split_advance: int, last_word_end=None):
    """Host only (AX_WHISPER_LongWordAdvance): the seek rule of long-form under word timestamps. ids: one window's ids (eot excluded),
    last_word_end: the end of the window's last word in file time, None without a word -> (advance in frames, whether the word end
    was taken)."""
    L = load_library()
    a = _i32(ids).reshape(-1)
    adv, by = C.c_int(), C.c_int()
    if L.AX_WHISPER_LongWordAdvance(a.ctypes.data_as(ip), len(a), int(timestamp_begin), int(seek), int(window_frames), int(split_advance),
                                    0 if last_word_end is None else 1, 0.0 if last_word_end is None else float(last_word_end),
                                    C.byref(adv), C.byref(by)) != 0:
        raise RuntimeError("AX_WHISPER_LongWordAdvance failed")
    return adv.value, bool(by.value)


def words_from_alignment(tokens_path: str, ids, eot: int, language: str, seg_tokens, seg_start, seg_end, jump, token_logprob,
                         last_speech_timestamp: float = 0.0, time_offset=None):
    """Host only (AX_WHISPER_WordsFromAlignment): the words of one window -> ([(segment, word bytes, start, end, probability)],
    seg_start, seg_end after the rule). time_offset (seconds; None: the call as it was): AX_WHISPER_WordsFromAlignmentAt, the window
    starts there in its file, and segment times, last_speech_timestamp and the words are in file time."""
    L = load_library()
    a, st_n = _i32(ids).reshape(-1), _i32(seg_tokens).reshape(-1)
    ss, se = np.array(seg_start, dtype=np.float64).reshape(-1), np.array(seg_end, dtype=np.float64).reshape(-1)
    j, lp = _i32(jump).reshape(-1), _f32(token_logprob).reshape(-1)
    if len(j) < len(a) + 1 or len(lp) < len(a) or len(ss) != len(st_n) or len(se) != len(st_n):
        raise ValueError("jump needs len(ids) + 1 entries, token_logprob len(ids), the segment arrays one entry per segment")
    n_max = len(a) + 1
    wseg, te = np.zeros(n_max, dtype=np.int32), np.zeros(n_max, dtype=np.int32)
    ws, we, wp = np.zeros(n_max, dtype=np.float64), np.zeros(n_max, dtype=np.float64), np.zeros(n_max, dtype=np.float32)
    n, nb, out = C.c_int(), C.c_int(), C.c_void_p()
    head = (os.fspath(tokens_path).encode(), a.ctypes.data_as(ip), len(a), int(eot), language.encode(), _ci(st_n), ss.ctypes.data_as(_dblp),
            se.ctypes.data_as(_dblp), len(st_n), _ci(j), lp.ctypes.data_as(fp), float(last_speech_timestamp))
    tail = (n_max, _ci(wseg), _ci(te), ws.ctypes.data_as(_dblp), we.ctypes.data_as(_dblp), wp.ctypes.data_as(fp), C.byref(n), C.byref(out), C.byref(nb))
    rc = L.AX_WHISPER_WordsFromAlignment(*head, *tail) if time_offset is None else L.AX_WHISPER_WordsFromAlignmentAt(*head, float(time_offset), *tail)
    if rc != 0:
        raise RuntimeError("AX_WHISPER_WordsFromAlignment failed: " + (L.AX_WHISPER_LastError(None) or b"").decode())
    texts = _word_texts(L, out, nb.value, te, n.value)
    return [(int(wseg[w]), texts[w], float(ws[w]), float(we[w]), np.float32(wp[w])) for w in range(n.value)], ss, se


def beam_finalize(hist, S, slot, pool_n, pool_ids, pool_len, pool_score, n: int):
    """Host only (AX_WHISPER_BeamFinalize): the fill and the ranking of beam search on the state after the loop. hist / pool_ids
    [clips*K][stride], S / slot / pool_len / pool_score [clips*K] (S, slot by rank), pool_n [clips]; n: the histories' length.
    Returns per clip a dict: ids, sum_logprob, avg_logprob, ended_eot, winner, records [(ids, score, from_pool)]."""
    L = load_library()
    hist, pool_ids = _i32(hist), _i32(pool_ids)
    S, pool_score = _f32(S).reshape(-1), _f32(pool_score).reshape(-1)
    slot, pool_n, pool_len = _i32(slot).reshape(-1), _i32(pool_n).reshape(-1), _i32(pool_len).reshape(-1)
    clips, slots = len(pool_n), len(S)
    K, stride = slots // max(clips, 1), hist.shape[-1]
    hist, pool_ids = hist.reshape(slots, stride), pool_ids.reshape(slots, stride)
    rec_ids = np.zeros((slots, stride), dtype=np.int32)
    rec_len, rec_pool = np.zeros(slots, dtype=np.int32), np.zeros(slots, dtype=np.int32)
    rec_score = np.zeros(slots, dtype=np.float32)
    n_rec, winner, n_ids, eot = (np.zeros(clips, dtype=np.int32) for _ in range(4))
    ids = np.zeros((clips, stride), dtype=np.int32)
    sum_lp, avg_lp = np.zeros(clips, dtype=np.float32), np.zeros(clips, dtype=np.float32)
    rc = L.AX_WHISPER_BeamFinalize(clips, K, int(n), stride, hist.ctypes.data_as(ip), S.ctypes.data_as(fp), slot.ctypes.data_as(_cip),
                                   pool_n.ctypes.data_as(_cip), pool_ids.ctypes.data_as(ip), pool_len.ctypes.data_as(_cip), pool_score.ctypes.data_as(fp),
                                   rec_ids.ctypes.data_as(ip), rec_len.ctypes.data_as(_cip), rec_score.ctypes.data_as(fp), rec_pool.ctypes.data_as(_cip),
                                   n_rec.ctypes.data_as(_cip), winner.ctypes.data_as(_cip), ids.ctypes.data_as(ip), n_ids.ctypes.data_as(_cip),
                                   sum_lp.ctypes.data_as(fp), avg_lp.ctypes.data_as(fp), eot.ctypes.data_as(_cip))
    if rc != 0:
        raise RuntimeError("AX_WHISPER_BeamFinalize failed: bad arguments")
    return [_beam_clip(c, K, ids, n_ids, sum_lp, avg_lp, eot, winner, rec_ids, rec_len, rec_score, rec_pool, n_rec) for c in range(clips)]


def _beam_clip(c, K, ids, n_ids, sum_lp, avg_lp, eot, winner, rec_ids, rec_len, rec_score, rec_pool, n_rec):
    recs = [(rec_ids[c * K + i, : rec_len[c * K + i]].tolist(), np.float32(rec_score[c * K + i]), bool(rec_pool[c * K + i])) for i in range(n_rec[c])]
    return dict(ids=ids[c, : n_ids[c]].tolist(), sum_logprob=np.float32(sum_lp[c]), avg_logprob=np.float32(avg_lp[c]), ended_eot=bool(eot[c]),
                winner=int(winner[c]), records=recs)


class Whisper:
    """Mirror of the reference's ``Whisper`` (python/whisper.py:54-99, cpp/src/Whisper.hpp:28-59)."""

    def __init__(self, model_type: str, model_path: str, language: str = "zh", device: int = -1, max_batch: int = 0, devices=None,
                 cross_kv: str | None = None):
        """devices: a list of HIP ordinals (or "all") -> one engine per device behind this handle (AX_WHISPER_InitMulti).
        cross_kv: "fp8" keeps the cross K/V as e4m3fn codes too and lets decoder steps of more than two clips read them (opt-in;
        DESIGN.md "FP8 cross K/V"); "h16" or None: the h16 images alone. The library reads the mode from AX_WHISPER_CROSS_KV while
        the handle is made: the variable is set for that call and put back afterwards, under a lock that every construction with a
        cross_kv argument takes (a handle made at the same moment on another thread WITHOUT the argument, or by other code through
        the C ABI, reads whatever the variable holds then)."""
        self.L = load_library()
        if cross_kv is None:
            self._init_handle(model_type, model_path, language, device, max_batch, devices)
        else:
            with _cross_kv_env_lock:
                before = os.environ.get("AX_WHISPER_CROSS_KV")
                os.environ["AX_WHISPER_CROSS_KV"] = str(cross_kv)
                try:
                    self._init_handle(model_type, model_path, language, device, max_batch, devices)
                finally:
                    if before is None:
                        del os.environ["AX_WHISPER_CROSS_KV"]
                    else:
                        os.environ["AX_WHISPER_CROSS_KV"] = before
        g = lambda k: self.L.AX_WHISPER_GetConfigInt(self.h, k.encode())
        self.n_mels, self.n_vocab, self.n_text_ctx = g("n_mels"), g("n_vocab"), g("n_text_ctx")
        self.n_text_layer, self.n_text_state, self.eot = g("n_text_layer"), g("n_text_state"), g("eot")
        self.sot_seq = [g(f"sot_seq{i}") for i in range(4)]
        self.timestamp_begin = g("timestamp_begin")
        self.no_speech = g("no_speech")
        self.n_devices = self.L.AX_WHISPER_GetDeviceCount(self.h)
        self._tokens_path = os.path.join(model_path, model_type, f"{model_type}-tokens.txt")

    def _init_handle(self, model_type, model_path, language, device, max_batch, devices):
        if devices is not None:
            if devices == "all":
                self.h = self.L.AX_WHISPER_InitMulti(model_type.encode(), model_path.encode(), language.encode(), None, 0, max_batch)
            else:
                arr = (C.c_int * len(devices))(*[int(d) for d in devices])
                self.h = self.L.AX_WHISPER_InitMulti(model_type.encode(), model_path.encode(), language.encode(), arr, len(devices), max_batch)
        else:
            self.h = self.L.AX_WHISPER_InitEx(model_type.encode(), model_path.encode(), language.encode(), device, max_batch)
        if not self.h:
            raise RuntimeError("AX_WHISPER_Init failed: " + (self.L.AX_WHISPER_LastError(None) or b"").decode())

    def get_config_int(self, key: str) -> int:
        """AX_WHISPER_GetConfigInt: a config file key, or one of the engine's own (include/ax_whisper_api.h)."""
        return self.L.AX_WHISPER_GetConfigInt(self.h, key.encode())

    @property
    def persistent_ts_launches(self) -> int:
        """One-clip timestamp and scored decodes of this handle that ran as ONE persistent launch under the timestamp rules and
        finished without a give-up (the route is on with AX_WHISPER_PERSIST_TS=1), summed over the handle's engines."""
        return self.get_config_int("persistent_ts_launches")

    def close(self):
        if getattr(self, "h", None):
            self.L.AX_WHISPER_Uninit(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: " + (self.L.AX_WHISPER_LastError(self.h) or b"").decode())

    def _take(self, p):
        s = C.string_at(p).decode("utf-8", errors="replace") if p else ""
        if p:
            self.L._free(p)
        return s

    # ---- legacy entry points ------------------------------------------------------------
    def run(self, audio, resample: bool = False) -> str:
        """PCM (16 kHz mono f32) or a wav path -> text (python/whisper.py:213-271). resample: a file is converted to 16 kHz by its own
        rate on the GPU first (AX_WHISPER_RunFileResampled); without it a file at another rate is fed as it is, with a warning."""
        out = C.c_void_p()
        if isinstance(audio, (str, os.PathLike)) and resample:
            self._check(self.L.AX_WHISPER_RunFileResampled(self.h, os.fspath(audio).encode(), C.byref(out)), "AX_WHISPER_RunFileResampled")
        elif isinstance(audio, (str, os.PathLike)):
            self._check(self.L.AX_WHISPER_RunFile(self.h, os.fspath(audio).encode(), C.byref(out)), "AX_WHISPER_RunFile")
        else:
            a = _f32(audio)
            self._check(self.L.AX_WHISPER_RunPCM(self.h, a.ctypes.data_as(fp), len(a), C.byref(out)), "AX_WHISPER_RunPCM")
        return self._take(out.value)

    # ---- additions ------------------------------------------------------------------------
    # what the clip-batch calls share: clips, lengths and budgets as the C ABI takes them; ids and scores as it fills them; the
    # dict per clip they come back as; the arrays of a teacher-forced decode
    @staticmethod
    def _clip_args(clips, max_new_clip=None):
        """-> (the clips as float32 arrays, which the pointers point into; B; pointers; lengths; per-clip budgets or None)"""
        clips = [_f32(c) for c in clips]
        B = len(clips)
        ptrs = (fp * B)(*[c.ctypes.data_as(fp) for c in clips])
        lens = (C.c_int * B)(*[len(c) for c in clips])
        mc = (C.c_int * B)(*[int(x) for x in max_new_clip]) if max_new_clip is not None else None
        return clips, B, ptrs, lens, mc

    def _score_buffers(self, B):
        """-> ((ids, n_ids, token_logprob, avg_logprob, no_speech_logprob, ended_eot), the same six as C arguments, in that order)"""
        ids = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        lp = np.zeros((B, self.n_text_ctx), dtype=np.float32)
        avg, nsp = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
        bufs = (ids, (C.c_int * B)(), lp, avg, nsp, (C.c_int * B)())
        return bufs, (ids.ctypes.data_as(ip), bufs[1], lp.ctypes.data_as(fp), avg.ctypes.data_as(fp), nsp.ctypes.data_as(fp), bufs[5])

    @staticmethod
    def _clip_dicts(bufs):
        ids, n, lp, avg, nsp, eot = bufs
        return [dict(ids=ids[b, : n[b]].tolist(), token_logprob=lp[b, : n[b] + 1].copy(), avg_logprob=float(avg[b]),
                     no_speech_logprob=float(nsp[b]), ended_eot=bool(eot[b])) for b in range(len(avg))]

    def _forced_buffers(self, batch, forced, want_logits):
        """-> ((logits [batch][n+1][n_vocab] or None, chosen, logprob [batch][n+1], no_speech_logprob [batch]), the forced ids and their
        count n as C arguments, those four as C arguments)"""
        f = np.ascontiguousarray(forced, dtype=np.int32).reshape(batch, -1)
        n = f.shape[1]
        logits = np.empty((batch, n + 1, self.n_vocab), dtype=np.float32) if want_logits else None
        ch = np.empty((batch, n + 1), dtype=np.int32)
        lp = np.empty((batch, n + 1), dtype=np.float32)
        nsp = np.empty(batch, dtype=np.float32)
        return ((logits, ch, lp, nsp), (f.ctypes.data_as(ip), n),
                (logits.ctypes.data_as(fp) if want_logits else None, ch.ctypes.data_as(ip), lp.ctypes.data_as(fp), nsp.ctypes.data_as(fp)))

    def run_tokens_batch(self, clips, max_new: int = 0):
        clips, B, ptrs, lens, _ = self._clip_args(clips)
        ids = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        n = (C.c_int * B)()
        self._check(self.L.AX_WHISPER_RunPCMBatchTokens(self.h, ptrs, lens, B, max_new, ids.ctypes.data_as(ip), n), "RunPCMBatchTokens")
        return [ids[b, : n[b]].tolist() for b in range(B)]

    def run_tokens(self, pcm, max_new: int = 0):
        return self.run_tokens_batch([pcm], max_new)[0]

    # ---- audio at any sample rate (DESIGN.md "Sample rates")
    def resample_batch(self, clips, rates):
        """The resample kernel alone: clips at rates[b] Hz -> their samples at 16 kHz (a clip at 16000 Hz comes back bit for bit)."""
        clips, B, ptrs, lens, _ = self._clip_args(clips)
        rt = (C.c_int * B)(*[int(r) for r in rates])
        outs = [np.empty(max(resampled_length(len(c), r), 1), dtype=np.float32) for c, r in zip(clips, rt)]
        optrs = (fp * B)(*[o.ctypes.data_as(fp) for o in outs])
        caps = (C.c_int * B)(*[len(o) for o in outs])
        n = (C.c_int * B)()
        self._check(self.L.AX_WHISPER_ResampleBatch(self.h, ptrs, lens, rt, B, optrs, caps, n), "ResampleBatch")
        return [o[: n[b]] for b, o in enumerate(outs)]

    def resample(self, audio, rate: int) -> np.ndarray:
        return self.resample_batch([audio], [rate])[0]

    def run_tokens_batch_rate(self, clips, rates, max_new: int = 0, timestamps: bool = False):
        """run_tokens_batch (timestamps: run_timestamp_tokens_batch) over clips at rates[b] Hz, resampled on the GPU behind their upload."""
        clips, B, ptrs, lens, _ = self._clip_args(clips)
        rt = (C.c_int * B)(*[int(r) for r in rates])
        ids = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        n = (C.c_int * B)()
        self._check(self.L.AX_WHISPER_RunPCMBatchRate(self.h, 1 if timestamps else 0, ptrs, lens, rt, B, max_new, ids.ctypes.data_as(ip), n),
                    "RunPCMBatchRate")
        return [ids[b, : n[b]].tolist() for b in range(B)]

    def load_audio_file_16k(self, path):
        """File decode + GPU resampling -> (mono f32 samples at 16 kHz, the file's sample rate, channels, samples per channel in the file)."""
        out, n, info = C.c_void_p(), C.c_int(), (C.c_int * 3)()
        self._check(self.L.AX_WHISPER_LoadAudioFile16k(self.h, os.fspath(path).encode(), C.byref(out), C.byref(n), info), "LoadAudioFile16k")
        a = np.ctypeslib.as_array(C.cast(out, fp), shape=(max(n.value, 1),))[: n.value].copy()
        self.L._free(out.value)
        return a, info[0], info[1], info[2]

    # ---- segment timestamps (timestamp mode: prefix [sot, lang, transcribe], Whisper's timestamp rules on the GPU)
    def run_timestamp_tokens_batch(self, clips, max_new: int = 0, max_new_clip=None):
        """ids per clip, timestamp tokens included (AX_WHISPER_RunPCMBatchTimestampTokens)."""
        clips, B, ptrs, lens, mc = self._clip_args(clips, max_new_clip)
        ids = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        n = (C.c_int * B)()
        self._check(self.L.AX_WHISPER_RunPCMBatchTimestampTokens(self.h, ptrs, lens, B, max_new, mc, ids.ctypes.data_as(ip), n),
                    "RunPCMBatchTimestampTokens")
        return [ids[b, : n[b]].tolist() for b in range(B)]

    # ---- confidence: timestamp mode + the log-probability of every decision and of <|nospeech|> (DESIGN.md "Confidence")
    def run_timestamp_scores_batch(self, clips, max_new: int = 0, max_new_clip=None):
        """Per clip a dict: ids (those of run_timestamp_tokens_batch), token_logprob (len(ids) + 1 values: one per id, then the
        decision that ended the clip), avg_logprob, no_speech_logprob, ended_eot (AX_WHISPER_RunPCMBatchTimestampScores)."""
        clips, B, ptrs, lens, mc = self._clip_args(clips, max_new_clip)
        bufs, out = self._score_buffers(B)
        self._check(self.L.AX_WHISPER_RunPCMBatchTimestampScores(self.h, ptrs, lens, B, max_new, mc, *out), "RunPCMBatchTimestampScores")
        return self._clip_dicts(bufs)

    # ---- prompt conditioning (DESIGN.md "Prompt conditioning"): prompts are id lists, an empty one means no prompt
    @staticmethod
    def _prompt_args(prompts):
        """-> (ids [batch][stride] as a C pointer, which keeps the array; stride; lengths); None: (None, 0, None), no prompts"""
        if prompts is None:
            return None, 0, None
        B = len(prompts)
        stride = max(1, max(len(p) for p in prompts))
        ids = np.zeros((B, stride), dtype=np.int32)
        for b, p in enumerate(prompts):
            ids[b, : len(p)] = np.asarray(p, dtype=np.int32)
        return ids.ctypes.data_as(ip), stride, (C.c_int * B)(*[len(p) for p in prompts])

    def run_timestamp_prompted_batch(self, clips, prompts, max_new: int = 0, max_new_clip=None):
        """run_timestamp_scores_batch with every clip conditioned on its prompt ids (AX_WHISPER_RunPCMBatchTimestampPrompted): the
        same dict per clip."""
        clips, B, ptrs, lens, mc = self._clip_args(clips, max_new_clip)
        if len(prompts) != B:
            raise ValueError("one prompt (possibly empty) per clip")
        bufs, out = self._score_buffers(B)
        self._check(self.L.AX_WHISPER_RunPCMBatchTimestampPrompted(self.h, ptrs, lens, B, max_new, mc, *self._prompt_args(prompts), *out),
                    "RunPCMBatchTimestampPrompted")
        return self._clip_dicts(bufs)

    def prefill_prompts(self, prompts, want_no_speech: bool = True, want_sot_logits: bool = False):
        """Stage level, after encode_mel of len(prompts) clips: reset + the prompted slots' context cached, `transcribe` about to be
        fed (AX_WHISPER_PrefillPrompts). Returns no_speech_logprob [batch] (0 for slots without a prompt) or None; with
        want_sot_logits (no_speech_logprob, sot_logits [batch][n_vocab]: the raw row the value was taken from)."""
        B = len(prompts)
        pid, stride, npr = self._prompt_args(prompts)
        nsp = np.zeros(B, dtype=np.float32) if want_no_speech or want_sot_logits else None
        rows = np.zeros((B, self.n_vocab), dtype=np.float32) if want_sot_logits else None
        self._check(self.L.AX_WHISPER_PrefillPrompts(self.h, B, pid, stride, npr, nsp.ctypes.data_as(fp) if nsp is not None else None,
                                                     rows.ctypes.data_as(fp) if want_sot_logits else None), "PrefillPrompts")
        return (nsp, rows) if want_sot_logits else nsp

    def get_self_kv(self, slot: int, n_rows: int):
        """Rows [0, n_rows) of the slot's self-attention cache -> (k, v), each fp32 [n_text_layer][n_rows][d]."""
        k = np.empty((self.n_text_layer, n_rows, self.n_text_state), dtype=np.float32)
        v = np.empty_like(k)
        self._check(self.L.AX_WHISPER_GetSelfKV(self.h, slot, n_rows, k.ctypes.data_as(fp), v.ctypes.data_as(fp)), "GetSelfKV")
        return k, v

    def get_persistent_self_kv(self, clip: int):
        """The self-attention cache of clip `clip` (1 or 2: its position in the last two- or three-clip persistent launch) ->
        (k, v), each fp32 [n_text_layer][512][d]: every block of every (layer, head), rows no step wrote included (zeros)."""
        k = np.empty((self.n_text_layer, 512, self.n_text_state), dtype=np.float32)
        v = np.empty_like(k)
        self._check(self.L.AX_WHISPER_GetPersistentSelfKV(self.h, clip, k.ctypes.data_as(fp), v.ctypes.data_as(fp)), "GetPersistentSelfKV")
        return k, v

    def decode_forced_timestamp_prompted(self, prompts, forced, want_logits: bool = True):
        """decode_forced_timestamp_scores under prompts (one non-empty prompt per clip): (logits [batch][n+1][n_vocab] or None, chosen,
        logprob [batch][n+1], no_speech_logprob [batch]); row i is the step that decides id i."""
        batch = len(prompts)
        bufs, fin, out = self._forced_buffers(batch, forced, want_logits)
        self._check(self.L.AX_WHISPER_DecodeForcedTimestampPrompted(self.h, batch, *self._prompt_args(prompts), *fin, *out), "DecodeForcedTimestampPrompted")
        return bufs

    # ---- language and task per clip (DESIGN.md "Language and task per clip"): a language is a code of the config's list, None (the
    # handle's language) or "auto" (detect it from the clip); a task is "transcribe" or "translate"
    @property
    def n_lang(self) -> int:
        return self.get_config_int("n_lang")

    def language_index(self, code: str) -> int:
        """AX_WHISPER_LanguageIndex: the index of a language code, -1 if the config does not list it."""
        return self.L.AX_WHISPER_LanguageIndex(self.h, code.encode())

    def language_code(self, index: int):
        """AX_WHISPER_LanguageCode: the code of language `index`, None outside the list."""
        c = self.L.AX_WHISPER_LanguageCode(self.h, int(index))
        return c.decode() if c is not None else None

    def _lang_args(self, B, languages, tasks):
        lang = task = None
        if languages is not None:
            if len(languages) != B:
                raise ValueError("one language (a code, None or \"auto\") per clip")
            v = []
            for x in languages:
                if isinstance(x, (int, np.integer)):  # an index as the C ABI takes it (-1 the handle's language, -2 detect)
                    v.append(int(x))
                    continue
                j = -1 if x is None else -2 if x == "auto" else self.language_index(x)
                if x is not None and x != "auto" and j < 0:
                    raise ValueError(f"unknown language {x!r}")
                v.append(j)
            lang = (C.c_int * B)(*v)
        if tasks is not None:
            if len(tasks) != B:
                raise ValueError("one task per clip")
            for t in tasks:
                if not isinstance(t, (int, np.integer)) and t not in (None, "transcribe", "translate"):
                    raise ValueError(f"unknown task {t!r}")
            # (an integer goes to the C ABI as it is: 0 transcribe, 1 translate)
            task = (C.c_int * B)(*[int(t) if isinstance(t, (int, np.integer)) else 1 if t == "translate" else 0 for t in tasks])
        return lang, task

    def detect_language(self, clips):
        """Front-end, encoder and detection only (AX_WHISPER_DetectLanguage): per clip (code, lang_logprob [n_lang])."""
        clips, B, ptrs, lens, _ = self._clip_args(clips)
        idx = (C.c_int * B)()
        lp = np.zeros((B, self.n_lang), dtype=np.float32)
        self._check(self.L.AX_WHISPER_DetectLanguage(self.h, ptrs, lens, B, idx, lp.ctypes.data_as(fp)), "DetectLanguage")
        return [(self.language_code(idx[b]), lp[b].copy()) for b in range(B)]

    def detect_language_stage(self, batch: int):
        """Stage level, after encode_mel: (index [batch], lang_logprob [batch][n_lang], lang_logit [batch][n_lang])."""
        idx = (C.c_int * batch)()
        lp = np.zeros((batch, self.n_lang), dtype=np.float32)
        lg = np.zeros((batch, self.n_lang), dtype=np.float32)
        self._check(self.L.AX_WHISPER_DetectLanguageStage(self.h, batch, idx, lp.ctypes.data_as(fp), lg.ctypes.data_as(fp)), "DetectLanguageStage")
        return np.array(idx[:], dtype=np.int32), lp, lg

    def language_logprob_rows(self, rows):
        """The detection kernel alone on residual rows [n][n_text_state]: (lang_logprob [n][n_lang], index [n], lang_logit [n][n_lang])."""
        x = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.n_text_state)
        n = x.shape[0]
        lp = np.zeros((n, self.n_lang), dtype=np.float32)
        lg = np.zeros((n, self.n_lang), dtype=np.float32)
        idx = (C.c_int * n)()
        self._check(self.L.AX_WHISPER_LanguageLogProbRows(self.h, x.ctypes.data_as(fp), n, lp.ctypes.data_as(fp), idx, lg.ctypes.data_as(fp)),
                    "LanguageLogProbRows")
        return lp, np.array(idx[:], dtype=np.int32), lg

    def run_timestamp_lang_batch(self, clips, languages=None, tasks=None, prompts=None, max_new: int = 0, max_new_clip=None):
        """run_timestamp_prompted_batch under a language and task per clip (AX_WHISPER_RunPCMBatchTimestampLang): the same dict per
        clip plus language (the code the clip was decoded under) and, for detecting clips, lang_logprob [n_lang]."""
        clips, B, ptrs, lens, mc = self._clip_args(clips, max_new_clip)
        if prompts is not None and len(prompts) != B:
            raise ValueError("one prompt (possibly empty) per clip")
        bufs, out = self._score_buffers(B)
        lout = (C.c_int * B)()
        llp = np.zeros((B, self.n_lang), dtype=np.float32)
        self._check(self.L.AX_WHISPER_RunPCMBatchTimestampLang(self.h, ptrs, lens, B, max_new, mc, *self._prompt_args(prompts),
                                                               *self._lang_args(B, languages, tasks), *out, lout, llp.ctypes.data_as(fp)),
                    "RunPCMBatchTimestampLang")
        res = self._clip_dicts(bufs)
        for b, o in enumerate(res):
            o["language"] = self.language_code(lout[b])
            if languages is not None and (languages[b] == "auto" or languages[b] == -2):
                o["lang_logprob"] = llp[b].copy()
        return res

    def prefill_contexts(self, batch: int, languages=None, tasks=None, prompts=None, want_no_speech: bool = True):
        """Stage level, after encode_mel of `batch` clips (AX_WHISPER_PrefillContexts): prefill_prompts under a language and task per
        clip. Returns (no_speech_logprob [batch] or None, language index [batch], lang_logprob [batch][n_lang])."""
        nsp = np.zeros(batch, dtype=np.float32) if want_no_speech else None
        lout = (C.c_int * batch)()
        llp = np.zeros((batch, self.n_lang), dtype=np.float32)
        self._check(self.L.AX_WHISPER_PrefillContexts(self.h, batch, *self._prompt_args(prompts), *self._lang_args(batch, languages, tasks),
                                                      nsp.ctypes.data_as(fp) if nsp is not None else None, None, lout, llp.ctypes.data_as(fp)),
                    "PrefillContexts")
        return nsp, np.array(lout[:], dtype=np.int32), llp

    def decode_forced_timestamp_lang(self, forced, languages=None, tasks=None, prompts=None, want_logits: bool = True):
        """decode_forced_timestamp_prompted under a language and task per clip, every clip behind its own context: (logits
        [batch][n+1][n_vocab] or None, chosen, logprob [batch][n+1], no_speech_logprob [batch], language index [batch])."""
        batch = np.shape(forced)[0]
        bufs, fin, out = self._forced_buffers(batch, forced, want_logits)
        lout = (C.c_int * batch)()
        self._check(self.L.AX_WHISPER_DecodeForcedTimestampLang(self.h, batch, *self._prompt_args(prompts), *self._lang_args(batch, languages, tasks),
                                                                *fin, *out, lout), "DecodeForcedTimestampLang")
        return (*bufs, np.array(lout[:], dtype=np.int32))

    def decode_forced_timestamp_scores(self, batch: int, forced, want_logits: bool = True, want_logits0: bool = True):
        """decode_forced_timestamps + (logprob [batch][n+1] of each step's chosen id, no_speech_logprob [batch], logits0
        [batch][n_vocab] or None: the raw row of decode offset 0). Returns (logits, chosen, logprob, no_speech_logprob, logits0)."""
        bufs, fin, out = self._forced_buffers(batch, forced, want_logits)
        l0 = np.empty((batch, self.n_vocab), dtype=np.float32) if want_logits0 else None
        self._check(self.L.AX_WHISPER_DecodeForcedTimestampScores(self.h, batch, *fin, *out, l0.ctypes.data_as(fp) if want_logits0 else None),
                    "DecodeForcedTimestampScores")
        return (*bufs, l0)

    def score_timestamp_rules(self, logits, histories):
        """The scored rules kernel alone: logits [batch][n_vocab], one id history per clip -> (chosen ids, their log-probabilities)."""
        lg = _f32(logits).reshape(-1, self.n_vocab)
        B = lg.shape[0]
        hist = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        nh = (C.c_int * B)()
        for b, h in enumerate(histories):
            hist[b, : len(h)] = h
            nh[b] = len(h)
        out = np.zeros(B, dtype=np.int32)
        lp = np.zeros(B, dtype=np.float32)
        self._check(self.L.AX_WHISPER_ScoreTimestampRules(self.h, lg.ctypes.data_as(fp), hist.ctypes.data_as(ip), nh, B, out.ctypes.data_as(ip),
                                                           lp.ctypes.data_as(fp)), "ScoreTimestampRules")
        return out.tolist(), lp

    def no_speech_logprob(self, logits) -> np.ndarray:
        """The no-speech kernel alone: logits [batch][n_vocab] -> log p(<|nospeech|>) over each whole row."""
        lg = _f32(logits).reshape(-1, self.n_vocab)
        out = np.zeros(lg.shape[0], dtype=np.float32)
        self._check(self.L.AX_WHISPER_NoSpeechLogProb(self.h, lg.ctypes.data_as(fp), lg.shape[0], out.ctypes.data_as(fp)), "NoSpeechLogProb")
        return out

    # ---- temperature fallback: seeded sampling in the rules kernel (DESIGN.md "Temperature fallback")
    @staticmethod
    def _sample_args(B, temperature, stream):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, dtype=np.float32), (B,)))
        st = np.ascontiguousarray(np.broadcast_to(np.asarray(stream, dtype=np.uint64), (B,)))
        return t, st

    def sample_timestamp_rules(self, logits, histories, temperature, stream, seed: int = 0):
        """The sampled rules kernel alone: score_timestamp_rules with a temperature and a stream id per clip (scalars are
        broadcast) and one seed -> (drawn ids, their untempered log-probabilities)."""
        lg = _f32(logits).reshape(-1, self.n_vocab)
        B = lg.shape[0]
        hist = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        nh = (C.c_int * B)()
        for b, h in enumerate(histories):
            hist[b, : len(h)] = h
            nh[b] = len(h)
        t, st = self._sample_args(B, temperature, stream)
        out = np.zeros(B, dtype=np.int32)
        lp = np.zeros(B, dtype=np.float32)
        self._check(self.L.AX_WHISPER_SampleTimestampRules(self.h, lg.ctypes.data_as(fp), hist.ctypes.data_as(ip), nh, B, t.ctypes.data_as(fp),
                                                            st.ctypes.data_as(C.POINTER(C.c_uint64)), int(seed), out.ctypes.data_as(ip),
                                                            lp.ctypes.data_as(fp)), "SampleTimestampRules")
        return out.tolist(), lp

    def decode_forced_timestamp_sampled(self, batch: int, forced, temperature, stream, seed: int = 0, want_logits: bool = True,
                                        want_logits0: bool = False):
        """decode_forced_timestamp_scores in sampled mode -> (logits, chosen, logprob, no_speech_logprob, logits0)."""
        bufs, fin, out = self._forced_buffers(batch, forced, want_logits)
        t, st = self._sample_args(batch, temperature, stream)
        l0 = np.empty((batch, self.n_vocab), dtype=np.float32) if want_logits0 else None
        self._check(self.L.AX_WHISPER_DecodeForcedTimestampSampled(self.h, batch, *fin, t.ctypes.data_as(fp), st.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                                   int(seed), *out, l0.ctypes.data_as(fp) if want_logits0 else None),
                    "DecodeForcedTimestampSampled")
        return (*bufs, l0)

    def run_timestamp_sampled_batch(self, clips, temperature, stream, seed: int = 0, max_new: int = 0, max_new_clip=None):
        """run_timestamp_scores_batch in sampled mode (AX_WHISPER_RunPCMBatchTimestampSampled): the same dict per clip."""
        clips, B, ptrs, lens, mc = self._clip_args(clips, max_new_clip)
        t, st = self._sample_args(B, temperature, stream)
        bufs, out = self._score_buffers(B)
        self._check(self.L.AX_WHISPER_RunPCMBatchTimestampSampled(self.h, ptrs, lens, B, max_new, mc, t.ctypes.data_as(fp),
                                                                  st.ctypes.data_as(C.POINTER(C.c_uint64)), int(seed), *out), "RunPCMBatchTimestampSampled")
        return self._clip_dicts(bufs)

    # ---- beam search (DESIGN.md "Beam search")
    def run_beam_batch(self, clips, beam_size: int = 5, max_new: int = 0):
        """Per clip a dict: ids (the winner's, timestamp tokens included, no eot), sum_logprob, avg_logprob, no_speech_logprob,
        ended_eot (AX_WHISPER_RunPCMBatchBeam). len(clips) * beam_size decoder slots must fit max_batch."""
        clips = [_f32(c) for c in clips]
        B = len(clips)
        ptrs = (fp * B)(*[c.ctypes.data_as(fp) for c in clips])
        lens = (C.c_int * B)(*[len(c) for c in clips])
        ids = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        n = (C.c_int * B)()
        sm, avg, nsp = (np.zeros(B, dtype=np.float32) for _ in range(3))
        eot = (C.c_int * B)()
        self._check(self.L.AX_WHISPER_RunPCMBatchBeam(self.h, ptrs, lens, B, int(beam_size), int(max_new), ids.ctypes.data_as(ip), n,
                                                      sm.ctypes.data_as(fp), avg.ctypes.data_as(fp), nsp.ctypes.data_as(fp), eot), "RunPCMBatchBeam")
        return [dict(ids=ids[b, : n[b]].tolist(), sum_logprob=np.float32(sm[b]), avg_logprob=np.float32(avg[b]),
                     no_speech_logprob=np.float32(nsp[b]), ended_eot=bool(eot[b])) for b in range(B)]

    def decode_beam(self, batch: int, beam_size: int, max_new: int = 0, trace: bool = False):
        """Stage level, after encode_mel of `batch` clips (AX_WHISPER_DecodeBeam). Returns (results, trace): results as
        run_beam_batch's plus winner and records [(ids, score, from_pool)]; trace is None, or a dict of arrays over the n_steps sampled
        steps and S = batch * beam_size slots: rows [n][S][n_vocab], cand_id / cand_logprob [n][S][K+1], n_cand [n][S], and after each
        step's selection S / slot [n][S] by rank, src / tok [n][S] by slot, pool_n [n][batch].
        With beam_size > 1 the call overwrites the encoded slots (clip c's cross K/V is copied into slots c*K .. c*K+K-1): call
        encode_mel again before any further decode_* call, decode_beam included. A trace holds max_new rows of S * n_vocab floats:
        give a budget with it."""
        K, B, Tc = int(beam_size), int(batch), self.n_text_ctx
        S = B * K
        budget = Tc - 3 if max_new <= 0 or max_new > Tc - 3 else int(max_new)
        ids = np.zeros((B, Tc), dtype=np.int32)
        n_ids, eot, n_rec, winner = (np.zeros(B, dtype=np.int32) for _ in range(4))
        sm, avg, nsp = (np.zeros(B, dtype=np.float32) for _ in range(3))
        rec_ids = np.zeros((max(S, 1), Tc), dtype=np.int32)
        rec_len, rec_pool = np.zeros(max(S, 1), dtype=np.int32), np.zeros(max(S, 1), dtype=np.int32)
        rec_score = np.zeros(max(S, 1), dtype=np.float32)
        n_steps = C.c_int()
        t = None
        if trace and S > 0 and 1 <= K <= 8:
            t = dict(rows=np.zeros((budget, S, self.n_vocab), dtype=np.float32), cand_id=np.zeros((budget, S, K + 1), dtype=np.int32),
                     cand_logprob=np.zeros((budget, S, K + 1), dtype=np.float32), n_cand=np.zeros((budget, S), dtype=np.int32),
                     S=np.zeros((budget, S), dtype=np.float32), slot=np.zeros((budget, S), dtype=np.int32), src=np.zeros((budget, S), dtype=np.int32),
                     tok=np.zeros((budget, S), dtype=np.int32), pool_n=np.zeros((budget, B), dtype=np.int32))
        pf = lambda k: t[k].ctypes.data_as(fp) if t else None
        pi = lambda k: t[k].ctypes.data_as(ip) if t else None
        self._check(self.L.AX_WHISPER_DecodeBeam(self.h, B, K, int(max_new), ids.ctypes.data_as(ip), n_ids.ctypes.data_as(_cip), sm.ctypes.data_as(fp),
                                                 avg.ctypes.data_as(fp), nsp.ctypes.data_as(fp), eot.ctypes.data_as(_cip), rec_ids.ctypes.data_as(ip),
                                                 rec_len.ctypes.data_as(_cip), rec_score.ctypes.data_as(fp), rec_pool.ctypes.data_as(_cip),
                                                 n_rec.ctypes.data_as(_cip), winner.ctypes.data_as(_cip), budget if t else 0, pf("rows"), pi("cand_id"),
                                                 pf("cand_logprob"), pi("n_cand"), pf("S"), pi("slot"), pi("src"), pi("tok"), pi("pool_n"),
                                                 C.byref(n_steps)), "DecodeBeam")
        out = []
        for c in range(B):
            r = _beam_clip(c, K, ids, n_ids, sm, avg, eot, winner, rec_ids, rec_len, rec_score, rec_pool, n_rec)
            r["no_speech_logprob"] = np.float32(nsp[c])
            out.append(r)
        if t:
            t = {k: v[: n_steps.value] for k, v in t.items()}
            t["n_steps"] = n_steps.value
        return out, t

    def beam_candidates(self, logits, histories, n_cand_max: int):
        """The candidates kernel alone: logits [rows][n_vocab], one id history per row -> (cand_id [rows][M], cand_logprob [rows][M],
        n_cand [rows]); entries from n_cand on are eot / -inf (AX_WHISPER_BeamCandidates)."""
        lg = _f32(logits).reshape(-1, self.n_vocab)
        B, M = lg.shape[0], int(n_cand_max)
        hist = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        nh = (C.c_int * B)()
        for b, h in enumerate(histories):
            hist[b, : len(h)] = h
            nh[b] = len(h)
        cid = np.zeros((B, max(M, 1)), dtype=np.int32)
        clp = np.zeros((B, max(M, 1)), dtype=np.float32)
        nc = np.zeros(B, dtype=np.int32)
        self._check(self.L.AX_WHISPER_BeamCandidates(self.h, lg.ctypes.data_as(fp), hist.ctypes.data_as(ip), nh, B, M, cid.ctypes.data_as(ip),
                                                     clp.ctypes.data_as(fp), nc.ctypes.data_as(_cip)), "BeamCandidates")
        return cid, clp, nc

    def beam_select(self, state: dict, cand_id, cand_logprob, n_cand, eot: int = None):
        """The selection kernel alone (AX_WHISPER_BeamSelect). state: dict(K, n, hist [S][stride], S, slot [S] by rank, pool_n [clips],
        pool_ids [S][stride], pool_len, pool_score [S], complete [clips]). Returns the new state (same keys, n + 1, hist with the
        chosen ids at index n — the reorder's copies are NOT applied) plus tok, src, slot_score [S] by slot and n_completed."""
        K, n = int(state["K"]), int(state["n"])
        hist, pool_ids = _i32(state["hist"]).copy(), _i32(state["pool_ids"]).copy()
        stride = hist.shape[-1]
        S, pool_score = _f32(state["S"]).reshape(-1).copy(), _f32(state["pool_score"]).reshape(-1).copy()
        slot, pool_n = _i32(state["slot"]).reshape(-1).copy(), _i32(state["pool_n"]).reshape(-1).copy()
        pool_len, complete = _i32(state["pool_len"]).reshape(-1).copy(), _i32(state["complete"]).reshape(-1).copy()
        clips, slots = len(pool_n), len(S)
        cid, clp, nc = _i32(cand_id).reshape(slots, -1), _f32(cand_logprob).reshape(slots, -1), _i32(n_cand).reshape(-1)
        tok, src = np.zeros(slots, dtype=np.int32), np.zeros(slots, dtype=np.int32)
        ss = np.zeros(slots, dtype=np.float32)
        done = C.c_int()
        self._check(self.L.AX_WHISPER_BeamSelect(self.h, clips, K, self.eot if eot is None else int(eot), n, stride, cid.ctypes.data_as(ip),
                                                 clp.ctypes.data_as(fp), nc.ctypes.data_as(_cip), hist.ctypes.data_as(ip), S.ctypes.data_as(fp),
                                                 slot.ctypes.data_as(_cip), pool_n.ctypes.data_as(_cip), pool_ids.ctypes.data_as(ip),
                                                 pool_len.ctypes.data_as(_cip), pool_score.ctypes.data_as(fp), complete.ctypes.data_as(_cip),
                                                 tok.ctypes.data_as(ip), src.ctypes.data_as(_cip), ss.ctypes.data_as(fp), C.byref(done)), "BeamSelect")
        hist = hist.reshape(slots, stride)
        complete_before = _i32(state["complete"]).reshape(-1)
        for s_ in range(slots):
            if not complete_before[s_ // K]:
                hist[s_, n] = tok[s_]
        return dict(K=K, n=n + 1, hist=hist, S=S, slot=slot, pool_n=pool_n, pool_ids=pool_ids.reshape(slots, stride), pool_len=pool_len,
                    pool_score=pool_score, complete=complete, tok=tok, src=src, slot_score=ss, n_completed=done.value)

    beam_finalize = staticmethod(beam_finalize)

    # ---- token suppression (DESIGN.md "Token suppression")
    def set_suppress_tokens(self, ids=None):
        """AX_WHISPER_SetSuppressTokens: the ids that every timestamp-mode decode of this handle treats as -inf; "non_speech": the
        list that openai-whisper's -1 stands for, from the model's tokens file; None or empty restores what the config file gave."""
        if isinstance(ids, str):
            if ids != "non_speech":
                raise ValueError('set_suppress_tokens: ids is a list of ids, None or "non_speech"')
            ids = non_speech_tokens(self._tokens_path)
        a = _i32(list(ids) if ids is not None else []).reshape(-1)
        self._check(self.L.AX_WHISPER_SetSuppressTokens(self.h, _ci(a) if len(a) else None, len(a)), "SetSuppressTokens")

    @property
    def suppress_tokens(self):
        """AX_WHISPER_GetSuppressTokens: the set in use, sorted."""
        n_max = max(self.get_config_int("n_suppress_tokens"), 1)
        ids, n = np.zeros(n_max, dtype=np.int32), C.c_int()
        self._check(self.L.AX_WHISPER_GetSuppressTokens(self.h, n_max, _ci(ids), C.byref(n)), "GetSuppressTokens")
        return [int(x) for x in ids[: n.value]]

    # ---- word-level timestamps (DESIGN.md "Word-level timestamps")
    def set_alignment_heads(self, pairs=None):
        """AX_WHISPER_SetAlignmentHeads: [(layer, head)]; None or empty restores what the handle was constructed with (the config file's
        "alignment_heads", else every head of the upper half of the layers)."""
        p = _i32(pairs if pairs else []).reshape(-1)
        self._check(self.L.AX_WHISPER_SetAlignmentHeads(self.h, _ci(p) if len(p) else None, len(p) // 2), "SetAlignmentHeads")

    def align_tokens(self, ids, num_frames, languages=None, tasks=None, want_matrix: bool = False):
        """Stage level, after encode_mel of len(ids) clips (AX_WHISPER_AlignTokens): per clip its text ids and its own mel frame count ->
        [dict(jump [n + 1], token_logprob [n], matrix [n + 5][frames // 2] if asked for)]. A clip without ids: empty arrays."""
        B = len(ids)
        stride = max(max((len(x) for x in ids), default=1), 1)
        a = np.zeros((B, stride), dtype=np.int32)
        for b, x in enumerate(ids):
            a[b, : len(x)] = x
        n = _i32([len(x) for x in ids])
        fr = _i32(num_frames).reshape(-1)
        if len(fr) != B:
            raise ValueError("one frame count per clip")
        lang, task = self._lang_args(B, languages, tasks)
        jump = np.zeros((B, stride + 1), dtype=np.int32)
        lp = np.zeros((B, stride), dtype=np.float32)
        m_rows, m_ld = stride + 5, max(int(fr.max()) // 2, 1)
        matrix = np.full((B, m_rows, m_ld), np.nan, dtype=np.float32) if want_matrix else None
        self._check(self.L.AX_WHISPER_AlignTokens(self.h, B, a.ctypes.data_as(ip), stride, _ci(n), _ci(fr), lang, task, _ci(jump), lp.ctypes.data_as(fp),
                                                  matrix.ctypes.data_as(fp) if want_matrix else None, m_rows, m_ld), "AlignTokens")
        out = []
        for b in range(B):
            k = int(n[b])
            o = dict(jump=jump[b, : k + 1].copy() if k else jump[b, :0].copy(), token_logprob=lp[b, :k].copy())
            if want_matrix:
                o["matrix"] = matrix[b, : k + 5, : int(fr[b]) // 2].copy() if k else matrix[b, :0, :0].copy()
            out.append(o)
        return out

    def vocab_logprob_rows(self, x, ids, route: str = "fused") -> np.ndarray:
        """The token probabilities alone (AX_WHISPER_VocabLogProbRows): x [rows][n_text_state] final residual rows, one id below eot per
        row -> float32 [rows], log p(id) over the ids below eot. route "fused": csrc/vocab_logprob.hip; "rows": the logits launch
        four rows at a time."""
        if route not in ("rows", "fused"):
            raise ValueError("route is rows or fused")
        x = _f32(x).reshape(-1, self.n_text_state)
        a = _i32(ids).reshape(-1)
        if len(a) != x.shape[0]:
            raise ValueError("one id per row")
        out = np.zeros(len(a), dtype=np.float32)
        self._check(self.L.AX_WHISPER_VocabLogProbRows(self.h, x.ctypes.data_as(fp), len(a), a.ctypes.data_as(ip), out.ctypes.data_as(fp),
                                                       1 if route == "fused" else 0), "VocabLogProbRows")
        return out

    def align_qk_softmax(self, q, k, row0, length, n_keys, slot, heads, rows_pad: int, f_pad: int, fill: float = np.nan):
        """align_qk_softmax_kernel alone (AX_WHISPER_AlignQKSoftmax): q [rows][64 n_head], k [n_slots][n_head][keys_pad][64] ->
        P [n_clips][len(heads)][rows_pad][f_pad], prefilled with `fill`."""
        q, k = _f32(q), _f32(k)
        n = len(length)
        P = np.full((n, len(heads), rows_pad, f_pad), fill, dtype=np.float32)
        ln, nk, r0, sl, hd = _i32(length), _i32(n_keys), _i32(row0), _i32(slot), _i32(heads)
        self._check(self.L.AX_WHISPER_AlignQKSoftmax(self.h, n, _ci(ln), _ci(nk), q.ctypes.data_as(fp), q.shape[0], k.shape[1], _ci(r0), k.ctypes.data_as(fp),
                                                     k.shape[0], k.shape[2], _ci(sl), _ci(hd), len(hd), P.ctypes.data_as(fp), rows_pad, f_pad),
                    "AlignQKSoftmax")
        return P

    def align_normalize(self, P, length, n_keys, matrix, inv_heads: float):
        """align_normalize_kernel alone (AX_WHISPER_AlignNormalize): P [n_clips][n_align][rows_pad][f_pad], matrix [n_clips][m_rows][m_ld]
        -> the matrix with the layer's contribution added."""
        P, m = _f32(P), _f32(matrix).copy()
        ln, nk = _i32(length), _i32(n_keys)
        self._check(self.L.AX_WHISPER_AlignNormalize(self.h, P.shape[0], _ci(ln), _ci(nk), P.ctypes.data_as(fp), P.shape[1], P.shape[2], P.shape[3],
                                                     float(inv_heads), m.ctypes.data_as(fp), m.shape[1], m.shape[2]), "AlignNormalize")
        return m

    def align_dtw(self, matrix, length, n_keys, fill: int = -1):
        """align_dtw_kernel alone (AX_WHISPER_AlignDTW): matrix [n_clips][m_rows][m_ld] -> jump [n_clips][m_rows] (length[c] - 4 entries
        per clip, the rest keeps `fill`)."""
        m = _f32(matrix)
        ln, nk = _i32(length), _i32(n_keys)
        jump = np.full((m.shape[0], m.shape[1]), fill, dtype=np.int32)
        self._check(self.L.AX_WHISPER_AlignDTW(self.h, m.shape[0], _ci(ln), _ci(nk), m.ctypes.data_as(fp), m.shape[1], m.shape[2], _ci(jump), jump.shape[1]),
                    "AlignDTW")
        return jump

    def run_word_timestamps_batch(self, clips, languages=None, tasks=None, max_new: int = 0):
        """AX_WHISPER_RunPCMBatchWordTimestamps: per clip dict(ids, text_ids (the aligned ids), language, segments [(start, end, text,
        [(word, start, end, probability)])], jump, token_logprob). Words are text decoded with errors="replace"; `words_bytes` holds them as bytes
        with their segment index."""
        clips, B, ptrs, lens, _ = self._clip_args(clips)
        lang, task = self._lang_args(B, languages, tasks)
        Tc = self.n_text_ctx
        ids = np.zeros((B, Tc), dtype=np.int32)
        n, lout, nseg, nw = (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)()
        ss, se = np.zeros((B, Tc), dtype=np.float64), np.zeros((B, Tc), dtype=np.float64)
        wseg, wte = np.zeros((B, Tc), dtype=np.int32), np.zeros((B, Tc), dtype=np.int32)
        ws, we, wp = np.zeros((B, Tc), dtype=np.float64), np.zeros((B, Tc), dtype=np.float64), np.zeros((B, Tc), dtype=np.float32)
        text = (C.c_void_p * B)()
        jump, lp = np.zeros((B, Tc), dtype=np.int32), np.zeros((B, Tc), dtype=np.float32)
        rc = self.L.AX_WHISPER_RunPCMBatchWordTimestamps(self.h, ptrs, lens, B, max_new, lang, task, ids.ctypes.data_as(ip), n, lout, Tc, nseg,
                                                         ss.ctypes.data_as(_dblp), se.ctypes.data_as(_dblp), nw, _ci(wseg), _ci(wte), ws.ctypes.data_as(_dblp),
                                                         we.ctypes.data_as(_dblp), wp.ctypes.data_as(fp), text, _ci(jump), lp.ctypes.data_as(fp))
        texts = []
        for b in range(B):  # (non-NULL entries are the caller's to free, also after a failure)
            out = C.c_void_p(text[b])
            texts.append(_word_texts(self.L, out, int(wte[b, nw[b] - 1]) if rc == 0 and nw[b] > 0 else 0, wte[b], nw[b] if rc == 0 else 0))
        self._check(rc, "RunPCMBatchWordTimestamps")
        res = []
        for b in range(B):
            row = ids[b, : n[b]]
            spans = split_segments(row.tolist(), self.timestamp_begin, self.eot, min(len(clips[b]) / 16000.0, 30.0))
            text_ids = [int(t) for (_, _, tb, te) in spans for t in row[tb:te] if t < self.eot][: Tc - 5]
            n_text = len(text_ids)
            wb = [(int(wseg[b, w]), texts[b][w], float(ws[b, w]), float(we[b, w]), np.float32(wp[b, w])) for w in range(nw[b])]
            segs = []
            for k in range(nseg[b]):
                words = [(t.decode("utf-8", errors="replace"), s, e, float(p)) for (sg, t, s, e, p) in wb if sg == k]
                segs.append((float(ss[b, k]), float(se[b, k]), "".join(w[0] for w in words), words))
            res.append(dict(ids=row.tolist(), text_ids=text_ids, language=self.language_code(lout[b]), segments=segs, words_bytes=wb,
                            jump=jump[b, : n_text + 1].copy(), token_logprob=lp[b, :n_text].copy()))
        return res

    def run_word_timestamps(self, audio, language=None):
        """One clip (PCM or a wav path) -> [(start, end, text, [(word, start, end, probability)])], openai-whisper's word_timestamps=True
        for one window; language: a code, None (the handle's) or "auto"."""
        if isinstance(audio, (str, os.PathLike)):
            audio, _, _ = load_audio_file(audio)
        return self.run_word_timestamps_batch([audio], None if language is None else [language])[0]["segments"]

    def segments(self, ids, num_samples: int):
        """[(start_s, end_s, text)] of one clip's timestamp-mode ids."""
        clip_s = min(num_samples / 16000.0, 30.0)
        return [(s, e, self.transcript(ids[tb:te])) for s, e, tb, te in split_segments(ids, self.timestamp_begin, self.eot, clip_s)]

    def run_timestamps(self, audio, max_new: int = 0, beam_size: int = 1):
        """PCM (16 kHz mono f32) -> [(start_s, end_s, text)], one entry per segment. beam_size > 1: of the beam search's winner."""
        a = _f32(audio)
        if beam_size > 1:
            return self.segments(self.run_beam_batch([a], beam_size, max_new)[0]["ids"], len(a))
        return self.segments(self.run_timestamp_tokens_batch([a], max_new)[0], len(a))

    # ---- long-form: audio longer than 30 s, seek over 30 s windows on the segment timestamps
    def compute_mel_window(self, pcm, seek: int) -> np.ndarray:
        """Whole-file front-end + window kernel: the [n_mels][3000] window at `seek` (frames of 10 ms) of one file."""
        a = _f32(pcm)
        out = np.empty((self.n_mels, 3000), dtype=np.float32)
        self._check(self.L.AX_WHISPER_ComputeMelWindow(self.h, a.ctypes.data_as(fp), len(a), int(seek), out.ctypes.data_as(fp)), "ComputeMelWindow")
        return out

    def run_long_windows(self, files, max_new: int = 0, max_passes: int = 0, no_speech_threshold=None, logprob_threshold=None, scores: bool = False,
                         compression_ratio_threshold=None, temperatures=None, seed: int = 0, file_ids=None, initial_prompt_ids=None,
                         condition_on_previous_text: bool = False, languages=None, tasks=None, word_timestamps=None):
        """The seek loop over `files` (PCM arrays), one window of every unfinished file per pass. Per file, the list of its
        decoded windows (seek, window_frames, advance, ids, pass, slot) in order. max_new: id budget per window;
        max_passes > 0 stops after that many passes (the slots then hold the last pass's cross K/V).
        With a threshold (the silent-window rule: a skipped window advances by its window_frames) or scores=True the call is the
        scored one and every tuple gains (no_speech_logprob, avg_logprob, skipped).
        With compression_ratio_threshold or temperatures the call is the fallback one (AX_WHISPER_RunPCMLongWindowsFallback;
        temperatures default to 0, 0.2, .. 1.0): every attempt is a tuple, which gains (attempt, temperature, compression_ratio,
        kept) after those three; there a missing logprob_threshold switches its part of the fallback rule off. file_ids: one id per
        file naming its random streams (default: its index in `files`); equal (seed, id) give a file the same windows in any call.
        With initial_prompt_ids (one id list per file, or None) or condition_on_previous_text the call is the prompted one
        (AX_WHISPER_RunPCMLongWindowsPrompted; scored, with fallback only if asked for as above): every tuple ends with the length of
        the prompt its window was conditioned on.
        With languages (per file a code, None or "auto") or tasks ("transcribe" / "translate") the call is
        AX_WHISPER_RunPCMLongWindowsLang, and the result is the pair (that list, the language code of every file); the tuples are
        those of the prompted call.
        word_timestamps (None: the calls above as they were; True / False): AX_WHISPER_RunPCMLongWindowsWords, whose result with
        False is the languages / tasks call's, and with True one more entry per window, a dict: text_ids, seg_tokens, jump,
        token_logprob (what was aligned and what the alignment gave), seg_start, seg_end (file time, after the word rule), words
        [(segment, word bytes, start, end, probability)] in file time, by_word_end (the advance is the word-end seek)."""
        files = [_f32(f) for f in files]
        o, keep, fallback = self._long_options(len(files), no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, seed,
                                               file_ids, initial_prompt_ids, condition_on_previous_text, languages, tasks, word_timestamps)
        per_lang = languages is not None or tasks is not None
        prompted = bool(condition_on_previous_text) or initial_prompt_ids is not None
        scored = scores or no_speech_threshold is not None or logprob_threshold is not None
        form = ("Words" if word_timestamps is not None else "Lang" if per_lang else "Prompted" if prompted else "Fallback" if fallback else
                "Scored" if scored else "")
        out, codes = self._long_windows(form, files, max_new, max_passes, o, fallback)
        return out if codes is None else (out, codes)

    def _long_options(self, n, no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, seed, file_ids, initial_prompt_ids,
                      condition_on_previous_text, languages, tasks, word_timestamps, logprob_nan: bool = False):
        """-> (AX_WHISPER_LONG_OPTIONS, what its pointers point into, whether the call has fallback): the option arguments of the
        long-form methods as the C ABI takes them; every legacy argument list is a part of this struct (_LONG_FORMS). None
        thresholds become the values that switch their comparison off (_thresholds); with fallback a missing logprob_threshold is
        NaN, which switches its part of the fallback rule off (logprob_nan: also without fallback, as the one-file Prompted and Lang
        text forms have always passed it)."""
        fallback = compression_ratio_threshold is not None or temperatures is not None
        nst, lpt = _thresholds(no_speech_threshold, logprob_threshold)
        if logprob_threshold is None and (fallback or logprob_nan):
            lpt = float("nan")
        crt = float("nan") if compression_ratio_threshold is None else float(compression_ratio_threshold)
        temps = _f32((DEFAULT_TEMPERATURES if temperatures is None else temperatures) if fallback else [])
        init = [[] if q is None else list(q) for q in (initial_prompt_ids if initial_prompt_ids is not None else [None] * n)]
        if len(init) != n:
            raise ValueError("one initial prompt (or None) per file")
        pid, stride, npr = self._prompt_args(init)
        lang, task = self._lang_args(n, languages, tasks)
        fid = (C.c_int * n)(*[int(x) for x in file_ids]) if file_ids is not None else None
        o = LongOptions(nst, lpt, crt, temps.ctypes.data_as(fp) if fallback else None, len(temps), int(seed), fid, pid, stride, npr,
                        int(bool(condition_on_previous_text)), lang, task, int(bool(word_timestamps)))
        return o, (temps, pid, npr, lang, task, fid), fallback

    def _long_windows(self, form, files, max_new, max_passes, o, fallback, chunk=None):
        """One window-log call, AX_WHISPER_RunPCMLongWindows<form> (with chunk, a ChunkOptions: AX_WHISPER_RunPCMLongChunkedWindows,
        form "" or "Scored") over `files` (float32 arrays) under the LongOptions `o` -> (per file the list of its windows, the
        language code of every file or None). The buffers hold `cap` windows; a call that decodes more says how many and is repeated.
        A window is (seek, window_frames, advance, ids, pass, slot), then what its form adds (run_long_windows)."""
        n, Tc, pi = len(files), self.n_text_ctx, C.POINTER(C.c_int)
        ptrs = (fp * n)(*[f.ctypes.data_as(fp) for f in files])
        lens = (C.c_int * n)(*[len(f) for f in files])
        name = "RunPCMLongChunkedWindows" if chunk is not None else "RunPCMLongWindowsWords" if form == "Words" else "RunPCMLongWindows"
        fn = getattr(self.L, "AX_WHISPER_" + (name if chunk is not None else "RunPCMLongWindows" + form))
        scored, prompted, per_lang, words = form != "", form in ("Prompted", "Lang", "Words"), form in ("Lang", "Words"), form == "Words" and bool(o.word_timestamps)
        # room for every window advancing fully, twice over (chunked: every window of the plan at its shortest)
        cap = sum(len(f) // 160 // 3000 + 2 for f in files) * 2 if chunk is None else sum(len(f) // 160 // max(chunk.min_frames, 1) + 2 for f in files)
        while True:
            info, ids, wp = np.zeros((cap, 7), dtype=np.int32), np.zeros((cap, Tc), dtype=np.int32), np.zeros(cap, dtype=np.int32)
            sc = np.zeros((cap, 7 if fallback else 3), dtype=np.float32)
            nw, lout = C.c_int(), (C.c_int * n)()
            outs = (cap, info.ctypes.data_as(pi), ids.ctypes.data_as(ip)) + ((sc.ctypes.data_as(fp),) if scored else (None,) if chunk is not None else ())
            outs += ((wp.ctypes.data_as(pi),) if prompted else ()) + (C.byref(nw),) + ((lout,) if per_lang else ())
            if form == "Words":
                m = cap * Tc  # (a window has fewer segments and words than ids)
                ww, tid, jmp = np.zeros((cap, 4), dtype=np.int32), np.zeros((cap, Tc), dtype=np.int32), np.zeros((cap, Tc + 1), dtype=np.int32)
                tlp = np.zeros((cap, Tc), dtype=np.float32)
                sgt, wsg, wte = (np.zeros(m, dtype=np.int32) for _ in range(3))
                sgs, sge, wst, wen = (np.zeros(m, dtype=np.float64) for _ in range(4))
                wpr = np.zeros(m, dtype=np.float32)
                log = LongWordLog(m, m, ww.ctypes.data_as(pi), tid.ctypes.data_as(ip), jmp.ctypes.data_as(pi), tlp.ctypes.data_as(fp), sgt.ctypes.data_as(pi),
                                  sgs.ctypes.data_as(_dblp), sge.ctypes.data_as(_dblp), wsg.ctypes.data_as(pi), wte.ctypes.data_as(pi),
                                  wst.ctypes.data_as(_dblp), wen.ctypes.data_as(_dblp), wpr.ctypes.data_as(fp), None)
                outs += (C.byref(log),)
            args = (C.byref(chunk), C.byref(o)) if chunk is not None else _LONG_FORMS[form](o)
            rc = fn(self.h, ptrs, lens, n, int(max_new), int(max_passes), *args, *outs)
            if form == "Words":
                text = C.string_at(log.text, int(wte[max(int(ww[: nw.value, 2].sum()) - 1, 0)])) if log.text and rc == 0 else b""
                if log.text:
                    self.L._free(log.text)
            if rc == 0:
                break
            msg = (self.L.AX_WHISPER_LastError(self.h) or b"").decode()
            need = re.search(r"(\d+) windows were decoded, win_cap is", msg)
            if not need:
                raise RuntimeError(name + " failed: " + msg)
            cap = int(need.group(1))
        out = [[] for _ in range(n)]
        sg = wd = 0
        for k in range(nw.value):
            f, seek, wf, adv, n_ids, pas, slot = (int(x) for x in info[k])
            w = (seek, wf, adv, ids[k, :n_ids].tolist(), pas, slot)
            if scored:
                w = w + (float(sc[k, 0]), float(sc[k, 1]), bool(sc[k, 2]))
            if fallback:
                w = w + (int(sc[k, 3]), float(sc[k, 4]), float(sc[k, 5]), bool(sc[k, 6]))
            if prompted:
                w = w + (int(wp[k]),)
            if words:
                nt, ns, nwd, by = (int(x) for x in ww[k])
                wl = [(int(wsg[j]), text[int(wte[j - 1]) if j else 0: int(wte[j])], float(wst[j]), float(wen[j]), np.float32(wpr[j])) for j in range(wd, wd + nwd)]
                w = w + (dict(text_ids=tid[k, :nt].tolist(), seg_tokens=sgt[sg: sg + ns].tolist(), jump=jmp[k, : nt + 1].copy() if nt else jmp[k, :0].copy(),
                              token_logprob=tlp[k, :nt].copy(), seg_start=sgs[sg: sg + ns].tolist(), seg_end=sge[sg: sg + ns].tolist(), words=wl,
                              by_word_end=bool(by)),)
                sg, wd = sg + ns, wd + nwd
            out[f].append(w)
        return out, [self.language_code(lout[f]) for f in range(n)] if per_lang else None


    def run_long_words(self, audio, no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None, temperatures=None, seed: int = 0,
                       initial_prompt_ids=None, condition_on_previous_text: bool = False, language=None, task=None):
        """PCM (16 kHz mono f32) or a wav path of any length -> [(start_s, end_s, text, [(word, start_s, end_s, probability)])], one entry
        per segment, times in the file (AX_WHISPER_RunPCMLongWords / RunFileLongWords): long-form transcription with word timestamps,
        under the thresholds, the temperature fallback, the prompt conditioning and the language / task of run_long_windows."""
        o, keep, _ = self._long_options(1, no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, seed, None,
                                        None if initial_prompt_ids is None else [initial_prompt_ids], condition_on_previous_text,
                                        None if language is None else [language], None if task is None else [task], True)
        r = LongWords()
        if isinstance(audio, (str, os.PathLike)):
            self._check(self.L.AX_WHISPER_RunFileLongWords(self.h, os.fspath(audio).encode(), C.byref(o), None, C.byref(r)), "RunFileLongWords")
        else:
            a = _f32(audio)
            self._check(self.L.AX_WHISPER_RunPCMLongWords(self.h, a.ctypes.data_as(fp), len(a), C.byref(o), None, C.byref(r)), "RunPCMLongWords")
        try:
            st = C.string_at(r.seg_text, r.seg_text_end[r.n_segments - 1]) if r.n_segments else b""
            wt = C.string_at(r.word_text, r.word_text_end[r.n_words - 1]) if r.n_words else b""
            out = [[r.seg_start[k], r.seg_end[k], st[(r.seg_text_end[k - 1] if k else 0): r.seg_text_end[k]].decode("utf-8", errors="replace"), []]
                   for k in range(r.n_segments)]
            for w in range(r.n_words):
                word = wt[(r.word_text_end[w - 1] if w else 0): r.word_text_end[w]].decode("utf-8", errors="replace")
                out[r.word_segment[w]][3].append((word, r.word_start[w], r.word_end[w], float(r.word_prob[w])))
            return [tuple(s) for s in out]
        finally:
            self.L.AX_WHISPER_FreeLongWords(C.byref(r))

    def transcript_lang(self, ids, language) -> str:
        """AX_WHISPER_TranscriptLang: the text of ids decoded under `language` (a code); the zh pass follows it, not the handle's."""
        a = _i32(ids)
        out = C.c_void_p()
        self._check(self.L.AX_WHISPER_TranscriptLang(self.h, a.ctypes.data_as(ip), len(a), self.language_index(language), C.byref(out)), "TranscriptLang")
        return self._take(out.value)

    def run_long_scored(self, audio, max_new: int = 0, no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None,
                        temperatures=None, seed: int = 0, initial_prompt_ids=None, condition_on_previous_text: bool = False, languages=None,
                        tasks=None):
        """run_long with confidence -> [(start_s, end_s, text, avg_logprob, no_speech_prob)]: every segment carries its window's two
        numbers (as openai-whisper reports them); windows the silent-window rule skips yield nothing. With
        compression_ratio_threshold or temperatures: under temperature fallback, the kept attempts only.
        With languages / tasks (a one-entry list each, or None): under that language and task; the result is then the pair (that list,
        the file's language code), and the text follows that language."""
        out = []
        wins = self.run_long_windows([audio], max_new, no_speech_threshold=no_speech_threshold, logprob_threshold=logprob_threshold, scores=True,
                                     compression_ratio_threshold=compression_ratio_threshold, temperatures=temperatures, seed=seed,
                                     initial_prompt_ids=None if initial_prompt_ids is None else [initial_prompt_ids],
                                     condition_on_previous_text=condition_on_previous_text, languages=languages, tasks=tasks)
        per_lang = languages is not None or tasks is not None
        code = wins[1][0] if per_lang else None
        for w in (wins[0] if per_lang else wins)[0]:
            seek, wf, _adv, ids, _p, _s, nsp, avg, skipped = w[:9]
            if skipped or (len(w) > 12 and not w[12]):
                continue
            for s, e, tb, te in split_window(ids, self.timestamp_begin, self.eot, wf)[0]:
                text = self.transcript_lang(ids[tb:te], code) if per_lang else self.transcript(ids[tb:te])
                out.append((seek * 0.01 + s, seek * 0.01 + e, text, avg, float(np.exp(np.float32(nsp)))))
        return (out, code) if per_lang else out

    def run_long(self, audio, max_new: int = 0):
        """PCM (16 kHz mono f32) of any length -> [(start_s, end_s, text)] with absolute times, one entry per segment."""
        out = []
        for seek, wf, _adv, ids, _p, _s in self.run_long_windows([audio], max_new)[0]:
            for s, e, tb, te in split_window(ids, self.timestamp_begin, self.eot, wf)[0]:
                out.append((seek * 0.01 + s, seek * 0.01 + e, self.transcript(ids[tb:te])))
        return out

    # ---- chunked long-form: the windows are chosen before decoding (cuts at quiet frames, on the GPU) and decoded side by side
    def long_frame_levels(self, files, smooth_frames: int = 25):
        """Whole-file front-end + levels kernel over `files` in one launch -> per file (e, s), float32 [1 + len // 160] each
        (AX_WHISPER_LongFrameLevels)."""
        files = [_f32(f) for f in files]
        n = len(files)
        ptrs = (fp * n)(*[f.ctypes.data_as(fp) for f in files])
        lens = (C.c_int * n)(*[len(f) for f in files])
        e = [np.empty(1 + len(f) // 160, dtype=np.float32) for f in files]
        s = [np.empty(1 + len(f) // 160, dtype=np.float32) for f in files]
        self._check(self.L.AX_WHISPER_LongFrameLevels(self.h, ptrs, lens, n, int(smooth_frames), (fp * n)(*[x.ctypes.data_as(fp) for x in e]),
                                                      (fp * n)(*[x.ctypes.data_as(fp) for x in s])), "LongFrameLevels")
        return list(zip(e, s))

    def long_cut_plan_from_levels(self, s, min_frames: int = 2000, max_frames: int = 3000):
        """The plan kernel alone on levels s [content] -> [(seek, len)] (AX_WHISPER_LongCutPlanFromLevels)."""
        a = _f32(s)
        cap = len(a) // max(int(min_frames), 1) + 2
        seek, ln, n = (C.c_int * cap)(), (C.c_int * cap)(), C.c_int()
        self._check(self.L.AX_WHISPER_LongCutPlanFromLevels(self.h, a.ctypes.data_as(fp), len(a), int(min_frames), int(max_frames), cap, seek, ln,
                                                            C.byref(n)), "LongCutPlanFromLevels")
        return [(seek[k], ln[k]) for k in range(n.value)]

    def long_cut_plan(self, files, min_frames: int = 2000, max_frames: int = 3000, smooth_frames: int = 25, levels: bool = False):
        """Front-end + levels + plan of `files` in one call -> per file [(seek, len)]; levels=True: the pair (that, per file the
        smoothed levels s the plan was made from) (AX_WHISPER_LongCutPlan)."""
        files = [_f32(f) for f in files]
        n = len(files)
        ptrs = (fp * n)(*[f.ctypes.data_as(fp) for f in files])
        lens = (C.c_int * n)(*[len(f) for f in files])
        cap = sum(len(f) // 160 // max(int(min_frames), 1) + 2 for f in files)
        chunk = ChunkOptions(int(max_frames), int(min_frames), int(smooth_frames), 1)
        nw, wf, ws, wl = (C.c_int * n)(), (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
        s = [np.empty(1 + len(f) // 160, dtype=np.float32) for f in files]
        self._check(self.L.AX_WHISPER_LongCutPlan(self.h, ptrs, lens, n, C.byref(chunk), cap, nw, wf, ws, wl,
                                                  (fp * n)(*[x.ctypes.data_as(fp) for x in s]) if levels else None), "LongCutPlan")
        out, k = [[] for _ in range(n)], 0
        for f in range(n):
            for _ in range(nw[f]):
                assert wf[k] == f
                out[f].append((ws[k], wl[k]))
                k += 1
        return (out, s) if levels else out

    def compute_mel_window_cut(self, pcm, seek: int, length: int) -> np.ndarray:
        """compute_mel_window for a window of `length` frames: zero from there on (AX_WHISPER_ComputeMelWindowCut)."""
        a = _f32(pcm)
        out = np.empty((self.n_mels, 3000), dtype=np.float32)
        self._check(self.L.AX_WHISPER_ComputeMelWindowCut(self.h, a.ctypes.data_as(fp), len(a), int(seek), int(length), out.ctypes.data_as(fp)),
                    "ComputeMelWindowCut")
        return out

    def run_long_chunked_windows(self, files, max_new: int = 0, max_passes: int = 0, min_frames: int = 2000, max_frames: int = 3000,
                                 smooth_frames: int = 25, no_speech_threshold=None, logprob_threshold=None, scores: bool = False, languages=None,
                                 tasks=None, beam_size: int = 1, **refused):
        """Chunked long-form over `files` (AX_WHISPER_RunPCMLongChunkedWindows): per file the list of its windows (seek, window_frames,
        advance, ids, pass, slot) in order, window_frames = advance = the window's length. With a threshold or scores=True the call is
        the scored one and every tuple gains (no_speech_logprob, avg_logprob, skipped). languages / tasks: per file, as in
        run_long_windows ("auto" is refused). refused: the options of run_long_windows this mode does not cover (temperatures,
        compression_ratio_threshold, initial_prompt_ids, condition_on_previous_text, word_timestamps); the library refuses them."""
        files = [_f32(f) for f in files]
        scored = scores or no_speech_threshold is not None or logprob_threshold is not None
        o, keep, _ = self._long_options(len(files), no_speech_threshold, logprob_threshold, refused.pop("compression_ratio_threshold", None),
                                        refused.pop("temperatures", None), 0, None, refused.pop("initial_prompt_ids", None),
                                        refused.pop("condition_on_previous_text", False), languages, tasks, refused.pop("word_timestamps", False))
        if refused:
            raise TypeError("unknown options: " + ", ".join(sorted(refused)))
        if no_speech_threshold is None and logprob_threshold is None:
            o.no_speech_threshold = o.logprob_threshold = float("nan")
        chunk = ChunkOptions(int(max_frames), int(min_frames), int(smooth_frames), int(beam_size))
        return self._long_windows("Scored" if scored else "", files, max_new, max_passes, o, False, chunk)[0]


    def run_long_chunked(self, audio, max_new: int = 0, min_frames: int = 2000, max_frames: int = 3000, smooth_frames: int = 25,
                         no_speech_threshold=None, logprob_threshold=None, language=None, task=None, **refused):
        """PCM (16 kHz mono f32) or an audio file of any length -> [(start_s, end_s, text)] in file time by chunked long-form: one
        entry per segment of every window (chunked_segments), without the windows the silent-window rule drops."""
        if isinstance(audio, (str, os.PathLike)):
            audio, _, _ = load_audio_file(audio)
        per_lang = language is not None or task is not None
        wins = self.run_long_chunked_windows([audio], max_new, 0, min_frames, max_frames, smooth_frames, no_speech_threshold, logprob_threshold,
                                             languages=[language] if per_lang else None, tasks=[task] if per_lang else None, **refused)[0]
        out = []
        for w in wins:
            seek, wf, _adv, ids = w[:4]
            if len(w) > 8 and w[8]:
                continue
            for s, e, tb, te in chunked_segments(ids, self.timestamp_begin, self.eot, seek, wf):
                text = self.transcript_lang(ids[tb:te], language) if language not in (None, -1) else self.transcript(ids[tb:te])
                out.append((s, e, text))
        return out

    def run_long_text(self, audio, no_speech_threshold=None, logprob_threshold=None, compression_ratio_threshold=None, temperatures=None,
                      seed: int = 0, initial_prompt_ids=None, condition_on_previous_text: bool = False, languages=None, tasks=None) -> str:
        """PCM or a wav path of any length -> the whole text (AX_WHISPER_RunPCMLong / RunFileLong; with a threshold: the *Opts
        forms, the text without the windows the silent-window rule skips; with compression_ratio_threshold or temperatures: the
        *Fallback forms; with condition_on_previous_text or a non-empty initial_prompt_ids: the *Prompted forms). With languages /
        tasks (a one-entry list each, or None): the *Lang forms, the text under that language and task (its zh pass follows the
        file's language)."""
        form = ("Lang" if languages is not None or tasks is not None else
                "Prompted" if condition_on_previous_text or (initial_prompt_ids is not None and len(initial_prompt_ids)) else
                "Fallback" if compression_ratio_threshold is not None or temperatures is not None else
                "Opts" if no_speech_threshold is not None or logprob_threshold is not None else "")
        o, keep, _ = self._long_options(1, no_speech_threshold, logprob_threshold, compression_ratio_threshold, temperatures, seed, None,
                                        None if initial_prompt_ids is None else [initial_prompt_ids], condition_on_previous_text, languages, tasks,
                                        False, logprob_nan=form in ("Prompted", "Lang"))
        out = C.c_void_p()
        if isinstance(audio, (str, os.PathLike)):
            name, head = "RunFileLong" + form, (os.fspath(audio).encode(),)
        else:
            a = _f32(audio)
            name, head = "RunPCMLong" + form, (a.ctypes.data_as(fp), len(a))
        self._check(getattr(self.L, "AX_WHISPER_" + name)(self.h, *head, *_LONG_TEXT_FORMS[form](o), C.byref(out)), name)
        return self._take(out.value)


    def decode_forced_timestamps(self, batch: int, forced, want_logits: bool = True):
        """Teacher-forced timestamp-mode decode of the EncodeMel slots -> (raw logits [batch][n+1][n_vocab] or None,
        chosen [batch][n+1]: the ids the rules pick at each step)."""
        f = np.ascontiguousarray(forced, dtype=np.int32).reshape(batch, -1)
        n = f.shape[1]
        logits = np.empty((batch, n + 1, self.n_vocab), dtype=np.float32) if want_logits else None
        ch = np.empty((batch, n + 1), dtype=np.int32)
        self._check(self.L.AX_WHISPER_DecodeForcedTimestamps(self.h, batch, f.ctypes.data_as(ip), n,
                                                             logits.ctypes.data_as(fp) if want_logits else None, ch.ctypes.data_as(ip)),
                    "DecodeForcedTimestamps")
        return logits, ch

    def apply_timestamp_rules(self, logits, histories):
        """The rules kernel alone: logits [batch][n_vocab], one id history per clip -> chosen id per clip."""
        lg = _f32(logits).reshape(-1, self.n_vocab)
        B = lg.shape[0]
        hist = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        nh = (C.c_int * B)()
        for b, h in enumerate(histories):
            hist[b, : len(h)] = h
            nh[b] = len(h)
        out = np.zeros(B, dtype=np.int32)
        self._check(self.L.AX_WHISPER_ApplyTimestampRules(self.h, lg.ctypes.data_as(fp), hist.ctypes.data_as(ip), nh, B,
                                                           out.ctypes.data_as(ip)), "ApplyTimestampRules")
        return out.tolist()

    def run_batch(self, clips):
        clips = [_f32(c) for c in clips]
        B = len(clips)
        ptrs = (fp * B)(*[c.ctypes.data_as(fp) for c in clips])
        lens = (C.c_int * B)(*[len(c) for c in clips])
        outs = (C.c_void_p * B)()
        self._check(self.L.AX_WHISPER_RunPCMBatch(self.h, ptrs, lens, B, outs), "RunPCMBatch")
        return [self._take(outs[b]) for b in range(B)]

    def run_device_tokens(self, d_ptr: int, stride: int, n_samples, max_new: int = 0, max_new_clip=None):
        """d_ptr: device address of [B][stride] f32 PCM already resident in HBM; max_new_clip: per-clip id budgets."""
        B = len(n_samples)
        lens = (C.c_int * B)(*[int(x) for x in n_samples])
        ids = np.zeros((B, self.n_text_ctx), dtype=np.int32)
        n = (C.c_int * B)()
        if max_new_clip is not None:
            mc = (C.c_int * B)(*[int(x) for x in max_new_clip])
            self._check(self.L.AX_WHISPER_RunDeviceBatchTokensRagged(self.h, C.c_void_p(d_ptr), stride, lens, B, max_new, mc, ids.ctypes.data_as(ip), n), "RunDeviceBatchTokensRagged")
            return [ids[b, : n[b]].tolist() for b in range(B)]
        self._check(self.L.AX_WHISPER_RunDeviceBatchTokens(self.h, C.c_void_p(d_ptr), stride, lens, B, max_new, ids.ctypes.data_as(ip), n), "RunDeviceBatchTokens")
        return [ids[b, : n[b]].tolist() for b in range(B)]

    def detokenize(self, ids) -> bytes:
        a = np.ascontiguousarray(ids, dtype=np.int32)
        out = C.c_void_p()
        self._check(self.L.AX_WHISPER_Detokenize(self.h, a.ctypes.data_as(ip), len(a), C.byref(out)), "Detokenize")
        b = C.string_at(out.value) if out.value else b""
        if out.value:
            self.L._free(out.value)
        return b

    def transcript(self, ids) -> str:
        a = np.ascontiguousarray(ids, dtype=np.int32)
        out = C.c_void_p()
        self._check(self.L.AX_WHISPER_Transcript(self.h, a.ctypes.data_as(ip), len(a), C.byref(out)), "Transcript")
        return self._take(out.value)

    def set_stream(self, stream_ptr: int):
        self._check(self.L.AX_WHISPER_SetStream(self.h, C.c_void_p(stream_ptr)), "SetStream")

    def compute_mel(self, pcm, rate: int = 16000) -> np.ndarray:
        a = _f32(pcm)
        out = np.empty((self.n_mels, 3000), dtype=np.float32)
        if rate == 16000:
            self._check(self.L.AX_WHISPER_ComputeMel(self.h, a.ctypes.data_as(fp), len(a), out.ctypes.data_as(fp)), "ComputeMel")
        else:
            self._check(self.L.AX_WHISPER_ComputeMelRate(self.h, a.ctypes.data_as(fp), len(a), int(rate), out.ctypes.data_as(fp)), "ComputeMelRate")
        return out

    def encode_mel(self, mel):
        m = _f32(mel)
        if m.ndim == 2:
            m = m[None]
        self._check(self.L.AX_WHISPER_EncodeMel(self.h, m.ctypes.data_as(fp), m.shape[0]), "EncodeMel")
        return m.shape[0]

    def get_cross_kv(self, slot: int = 0):
        shape = (self.n_text_layer, 1500, self.n_text_state)
        k, v = np.empty(shape, dtype=np.float32), np.empty(shape, dtype=np.float32)
        self._check(self.L.AX_WHISPER_GetCrossKV(self.h, slot, k.ctypes.data_as(fp), v.ctypes.data_as(fp)), "GetCrossKV")
        return k, v

    def get_cross_kv_fp8(self, slot: int = 0):
        """A cross_kv="fp8" handle's stored codes and scales of `slot`: (k_codes, v_codes) uint8 [n_text_layer][1500][n_text_state], raw
        e4m3fn bytes, and scales float32 [n_text_layer][n_text_head][2][64] (K's 64, then V's); value = code * scale."""
        shape = (self.n_text_layer, 1500, self.n_text_state)
        k, v = np.empty(shape, dtype=np.uint8), np.empty(shape, dtype=np.uint8)
        sc = np.empty((self.n_text_layer, self.n_text_state // 64, 2, 64), dtype=np.float32)
        u8 = C.POINTER(C.c_uint8)
        self._check(self.L.AX_WHISPER_GetCrossKVFp8(self.h, slot, k.ctypes.data_as(u8), v.ctypes.data_as(u8), sc.ctypes.data_as(fp)), "GetCrossKVFp8")
        return k, v, sc

    def cross_kv_quantize(self):
        """The quantise kernel alone over every slot of a cross_kv="fp8" handle (the h16 images as they stand -> codes and scales)."""
        self._check(self.L.AX_WHISPER_CrossKVQuantize(self.h), "CrossKVQuantize")

    def scan_stored16(self, batch: int = 1):
        """{buffer name: (non-finite elements, max finite |x|)} over every 16-bit tensor the engine stores between kernels."""
        n_max = 32
        names = C.create_string_buffer(32 * n_max)
        bad = (C.c_int64 * n_max)()
        mx = (C.c_float * n_max)()
        n = C.c_int()
        self._check(self.L.AX_WHISPER_ScanStored16(self.h, batch, n_max, names, bad, mx, C.byref(n)), "ScanStored16")
        return {names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode(): (int(bad[i]), float(mx[i])) for i in range(n.value)}

    def decode_forced(self, batch: int, forced, want_logits: bool = True):
        f = np.ascontiguousarray(forced, dtype=np.int32).reshape(batch, -1)
        n = f.shape[1]
        logits = np.empty((batch, n + 1, self.n_vocab), dtype=np.float32) if want_logits else None
        am = np.empty((batch, n + 1), dtype=np.int32)
        self._check(self.L.AX_WHISPER_DecodeForced(self.h, batch, f.ctypes.data_as(ip), n,
                                                   logits.ctypes.data_as(fp) if want_logits else None, am.ctypes.data_as(ip)), "DecodeForced")
        return logits, am

    def decode_greedy(self, batch: int, max_new: int = 0, max_new_clip=None):
        ids = np.zeros((batch, self.n_text_ctx), dtype=np.int32)
        n = (C.c_int * batch)()
        if max_new_clip is None:
            self._check(self.L.AX_WHISPER_DecodeGreedy(self.h, batch, max_new, ids.ctypes.data_as(ip), n), "DecodeGreedy")
        else:
            mc = (C.c_int * batch)(*[int(x) for x in max_new_clip])
            self._check(self.L.AX_WHISPER_DecodeGreedyRagged(self.h, batch, max_new, mc, ids.ctypes.data_as(ip), n), "DecodeGreedyRagged")
        return [ids[b, : n[b]].tolist() for b in range(batch)]

    # ---- utterance slots refilled while the others decode (AX_WHISPER_Stream*)
    def stream_open(self, n_slots: int, timestamps: bool = False):
        """timestamps: the scored timestamp mode (AX_WHISPER_StreamOpenMode, mode 1; an integer is passed on as the mode)."""
        if timestamps is False:
            self._check(self.L.AX_WHISPER_StreamOpen(self.h, n_slots), "StreamOpen")
        else:
            self._check(self.L.AX_WHISPER_StreamOpenMode(self.h, n_slots, 1 if timestamps is True else int(timestamps)), "StreamOpenMode")
        self._n_slots = n_slots

    def stream_admit(self, slot: int, pcm, max_new: int = 0, language=None, task=None):
        """language (a code, None or "auto") and task ("transcribe" / "translate"): a stream opened with timestamps=True."""
        if language is None and task is None:
            a = _f32(pcm)
            self._check(self.L.AX_WHISPER_StreamAdmit(self.h, slot, a.ctypes.data_as(fp), len(a), max_new), "StreamAdmit")
        else:
            self.stream_admit_batch([slot], [pcm], [max_new], languages=[language], tasks=None if task is None else [task])

    def stream_admit_batch(self, slots, clips, max_new=None, rates=None, languages=None, tasks=None):
        clips = [_f32(c) for c in clips]
        n = len(clips)
        sl = (C.c_int * n)(*[int(x) for x in slots])
        ptrs = (fp * n)(*[c.ctypes.data_as(fp) for c in clips])
        lens = (C.c_int * n)(*[len(c) for c in clips])
        mn = (C.c_int * n)(*[int(x) for x in max_new]) if max_new is not None else None
        if languages is not None or tasks is not None:
            lang, task = self._lang_args(n, languages, tasks)
            rt = (C.c_int * n)(*[int(r) for r in rates]) if rates is not None else None
            self._check(self.L.AX_WHISPER_StreamAdmitBatchLang(self.h, sl, ptrs, lens, rt, mn, lang, task, n), "StreamAdmitBatchLang")
        elif rates is None:
            self._check(self.L.AX_WHISPER_StreamAdmitBatch(self.h, sl, ptrs, lens, mn, n), "StreamAdmitBatch")
        else:
            rt = (C.c_int * n)(*[int(r) for r in rates])
            self._check(self.L.AX_WHISPER_StreamAdmitBatchRate(self.h, sl, ptrs, lens, rt, mn, n), "StreamAdmitBatchRate")

    def stream_step(self, n_steps: int = 8):
        fin = (C.c_int * max(self._n_slots, 3))()
        n = C.c_int()
        self._check(self.L.AX_WHISPER_StreamStep(self.h, n_steps, fin, C.byref(n)), "StreamStep")
        return [fin[i] for i in range(n.value)]

    def stream_collect(self, slot: int):
        ids = np.zeros(self.n_text_ctx, dtype=np.int32)
        n = C.c_int()
        self._check(self.L.AX_WHISPER_StreamCollect(self.h, slot, ids.ctypes.data_as(ip), C.byref(n)), "StreamCollect")
        return ids[: n.value].tolist()

    def stream_collect_scored(self, slot: int):
        """A finished slot of a timestamp-mode stream: dict(ids, token_logprob [n_ids + 1], avg_logprob, no_speech_logprob, ended_eot,
        language (the code the clip was decoded under), lang_index, lang_logprob [n_lang]: a detecting clip's, zeros otherwise)."""
        ids = np.zeros(self.n_text_ctx, dtype=np.int32)
        lp = np.zeros(self.n_text_ctx, dtype=np.float32)
        llp = np.zeros(self.n_lang, dtype=np.float32)
        n, eot, lang = C.c_int(), C.c_int(), C.c_int()
        avg, nsp = C.c_float(), C.c_float()
        self._check(self.L.AX_WHISPER_StreamCollectScored(self.h, slot, ids.ctypes.data_as(ip), C.byref(n), lp.ctypes.data_as(fp),
                                                           C.cast(C.byref(avg), fp), C.cast(C.byref(nsp), fp), C.byref(eot), C.byref(lang),
                                                           llp.ctypes.data_as(fp)), "StreamCollectScored")
        return dict(ids=ids[: n.value].tolist(), token_logprob=lp[: min(n.value + 1, self.n_text_ctx)].copy(), avg_logprob=avg.value,
                    no_speech_logprob=nsp.value, ended_eot=bool(eot.value), language=self.language_code(lang.value), lang_index=lang.value,
                    lang_logprob=llp)

    def stream_rules_stage(self, rows, off, done, detect, histories, slot_ctx, sentinel: float = -7.0, sentinel_int: int = -7):
        """The stream's rules kernel alone (AX_WHISPER_StreamRulesStage) on rows [n][n_vocab], off / done / detect [n], one id history per
        slot and slot_ctx [n][4]. Every output starts as a sentinel and is written only where the kernel writes: dict(chosen, logprob,
        no_speech, slot_ctx, lang_out, lang_logprob [n][n_lang])."""
        lg = _f32(rows).reshape(-1, self.n_vocab)
        n = lg.shape[0]
        hist = np.zeros((n, self.n_text_ctx), dtype=np.int32)
        nh = (C.c_int * n)()
        for b, h in enumerate(histories):
            hist[b, : len(h)] = h
            nh[b] = len(h)
        ctx = np.ascontiguousarray(slot_ctx, dtype=np.int32).reshape(n, 4).copy()
        chosen = np.full(n, sentinel_int, dtype=np.int32)
        lang = np.full(n, sentinel_int, dtype=np.int32)
        lp = np.full(n, sentinel, dtype=np.float32)
        nsp = np.full(n, sentinel, dtype=np.float32)
        llp = np.full((n, self.n_lang), sentinel, dtype=np.float32)
        ci = lambda a: (C.c_int * n)(*[int(x) for x in a])
        cp = C.POINTER(C.c_int)
        self._check(self.L.AX_WHISPER_StreamRulesStage(self.h, n, lg.ctypes.data_as(fp), ci(off), ci(done), ci(detect), hist.ctypes.data_as(ip), nh,
                                                        ctx.ctypes.data_as(cp), chosen.ctypes.data_as(ip), lp.ctypes.data_as(fp), nsp.ctypes.data_as(fp),
                                                        lang.ctypes.data_as(cp), llp.ctypes.data_as(fp)), "StreamRulesStage")
        return dict(chosen=chosen, logprob=lp, no_speech=nsp, slot_ctx=ctx, lang_out=lang, lang_logprob=llp)

    def stream_close(self):
        self._check(self.L.AX_WHISPER_StreamClose(self.h), "StreamClose")

    def run_stream_timestamps(self, clips, n_slots: int, max_new=0, languages=None, tasks=None, steps_per_call: int = 8):
        """`clips` through n_slots refillable slots in the scored timestamp mode, in arrival order; max_new: one budget or one per clip;
        languages / tasks: one per clip, as run_timestamp_lang_batch takes them. Per clip (segments, ids, token_logprobs, avg_logprob,
        no_speech_logprob, language, lang_logprob): segments [(start, end, text)] by split_segments with the text under the slot's
        language (transcript_lang), lang_logprob for detecting clips and None otherwise."""
        N = len(clips)
        budgets = list(max_new) if hasattr(max_new, "__len__") else [max_new] * N
        if languages is not None and len(languages) != N:
            raise ValueError("one language (a code, None or \"auto\") per clip")
        if tasks is not None and len(tasks) != N:
            raise ValueError("one task per clip")
        self.stream_open(n_slots, timestamps=True)
        try:
            out = [None] * N
            owner = {}
            free = list(range(n_slots))
            nxt = 0
            while nxt < N or owner:
                k = min(len(free), N - nxt)
                if k > 0:
                    self.stream_admit_batch(free[:k], clips[nxt:nxt + k], budgets[nxt:nxt + k],
                                            languages=None if languages is None else languages[nxt:nxt + k],
                                            tasks=None if tasks is None else tasks[nxt:nxt + k])
                for i in range(k):
                    owner[free.pop(0)] = nxt
                    nxt += 1
                for sl in self.stream_step(steps_per_call):
                    if sl not in owner:
                        continue
                    c = owner.pop(sl)
                    r = self.stream_collect_scored(sl)
                    free.append(sl)
                    clip_s = min(len(clips[c]) / 16000.0, 30.0)
                    segs = [(a, b, self.transcript_lang(r["ids"][t0:t1], r["language"]))
                            for a, b, t0, t1 in split_segments(r["ids"], self.timestamp_begin, self.eot, clip_s)]
                    detected = languages is not None and (languages[c] == "auto" or languages[c] == -2)
                    out[c] = (segs, r["ids"], r["token_logprob"], r["avg_logprob"], r["no_speech_logprob"], r["language"],
                              r["lang_logprob"] if detected else None)
            return out
        finally:
            self.stream_close()

    def run_stream(self, clips, n_slots: int, max_new=0, steps_per_call: int = 8, min_admit: int = 1, stamps=None):
        """Feed `clips` through n_slots refillable slots in arrival order; max_new: one budget or one per clip.
        min_admit: free slots to wait for before an admission pass (a larger encoder batch per pass; the last clips are
        admitted as they come). stamps: a list that receives time.perf_counter() of every collected clip, in completion order.
        Returns (ids per clip, decoder-step calls made)."""
        budgets = list(max_new) if hasattr(max_new, "__len__") else [max_new] * len(clips)
        self.stream_open(n_slots)
        try:
            out = [None] * len(clips)
            owner = {}
            free = list(range(n_slots))
            nxt = calls = 0
            while nxt < len(clips) or owner:
                k = min(len(free), len(clips) - nxt)
                if k < min(min_admit, len(clips) - nxt) and owner:
                    k = 0  # wait for more slots to free up (something is still decoding)
                if k == 1:
                    self.stream_admit(free[0], clips[nxt], budgets[nxt])
                elif k > 1:  # every free slot is refilled by ONE batched front-end + encoder pass
                    self.stream_admit_batch(free[:k], clips[nxt:nxt + k], budgets[nxt:nxt + k])
                for i in range(k):
                    owner[free.pop(0)] = nxt
                    nxt += 1
                calls += 1
                for sl in self.stream_step(steps_per_call):
                    if sl in owner:
                        out[owner.pop(sl)] = self.stream_collect(sl)
                        free.append(sl)
                        if stamps is not None:
                            stamps.append(time.perf_counter())
            return out, calls
        finally:
            self.stream_close()

    def timings(self):
        t = (C.c_float * 5)()
        self._check(self.L.AX_WHISPER_GetTimings(self.h, t), "GetTimings")
        return dict(frontend_ms=t[0], encoder_ms=t[1], decode_ms=t[2], wall_ms=t[3], steps=int(t[4]))

    def bench(self, what: str, batch: int = 1, arg: int = 0, iters: int = 10) -> float:
        ms = C.c_float()
        self._check(self.L.AX_WHISPER_Bench(self.h, what.encode(), batch, arg, iters, C.byref(ms)), "Bench")
        return ms.value
